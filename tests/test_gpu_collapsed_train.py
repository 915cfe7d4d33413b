"""-m gpu: training a DGP_Collapsed through all its layers.  compute_log_likelihood_gradients(inner=True) against the torch yardstick of
tests/collapsed_train_reference.py (bound rtol 1e-9, every pair within 1e-7 of its parameter's largest entry) and against central
differences of the device's own bound; ScipyOptimizer(inner=True); CollapsedAdamOptimizer."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import collapsed_train_reference as T

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _names(model):
    """id(Parameter) -> the oracle's state key (inner layers) or the yardstick's top key"""
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    top, names = model.layers[-1], {}
    for l, layer in enumerate(model.layers[:-1]):
        stat, wk = split_kernel(layer.kern)
        names.update({id(layer.feature.Z): f"l{l}.Z", id(layer.q_mu): f"l{l}.q_mu", id(layer.q_sqrt): f"l{l}.q_sqrt",
                      id(stat.variance): f"l{l}.kern_variance_raw", id(stat.lengthscales): f"l{l}.kern_lengthscales_raw"})
        if wk is not None:
            names[id(wk.variance)] = f"l{l}.white_variance_raw"
    names.update({id(top.feature.Z): "Z", id(top.kern.variance): "variance", id(top.kern.lengthscales): "lengthscales",
                  id(model.likelihood.likelihood.variance): "lik_variance"})
    return names


@pytest.mark.parametrize("name", ["two", "three", "white"])
def test_inner_gradients_against_the_yardstick(name):
    c = T.case(name)
    val, g_state, g_top, _, _ = T.reference(name)
    model = c.collapsed_model()
    zs = c.zs if name != "two" else None                    # one inner layer: its mean and variance depend on no draw
    bound, pairs, adj = model.compute_log_likelihood_gradients(zs=zs, inner=True)
    assert_allclose(bound, val, rtol=1e-9)
    names = _names(model)
    assert [names[id(p)] for p, _ in pairs[:4]] == ["Z", "variance", "lengthscales", "lik_variance"]
    want = [k for k in c.state if k != "lik_variance_raw"]
    assert sorted(names[id(p)] for p, _ in pairs[4:]) == sorted(want)
    worst = {}
    for p, g in pairs:
        key = names[id(p)]
        assert g.shape == p.shape
        ref = np.reshape(g_top[key], p.shape) if key in g_top else T.constrained_gradient(key, g_state[key], c.state[key]).reshape(p.shape)
        worst[key] = float(np.max(np.abs(g - ref)) / (np.max(np.abs(ref)) + 1e-12))
        if key.endswith("q_sqrt"):
            assert np.array_equal(np.triu(g, 1), np.zeros_like(g))
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= 1e-7}
    assert not bad, f"gradient mismatch (relative to the largest entry): {bad}"
    # the four pairs of the collapsed layer are those of the call without the inner layers, and the bound is compute_log_likelihood's
    bound4, pairs4, adj4 = model.compute_log_likelihood_gradients(zs=zs)
    for (p, g), (p4, g4) in zip(pairs[:4], pairs4):
        assert p is p4 and np.array_equal(_bits(g), _bits(g4)), names[id(p)]
    assert bound == bound4 == model.compute_log_likelihood(zs=zs)
    assert np.array_equal(_bits(adj["X_mean"]), _bits(adj4["X_mean"])) and adj["X_var"].shape == (c.N, c.X.shape[1])


def test_one_layer_model_returns_the_same_with_and_without_inner():
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    c = T.case("two")
    top = SGPR_Layer(RBF(2, variance=1.2, lengthscales=1.1), c.top["Z"].copy(), 1, Zero())
    model = DGP_Collapsed(c.X, c.Y, Gaussian(variance=0.1), [top])
    b0, p0, a0 = model.compute_log_likelihood_gradients()
    b1, p1, a1 = model.compute_log_likelihood_gradients(inner=True)
    assert b0 == b1 and len(p0) == len(p1) == 4
    for (q0, g0), (q1, g1) in zip(p0, p1):
        assert q0 is q1 and np.array_equal(_bits(g0), _bits(g1))
    assert np.array_equal(_bits(a0["X_mean"]), _bits(a1["X_mean"])) and np.array_equal(_bits(a0["X_var"]), _bits(a1["X_var"]))


def test_inner_gradients_against_central_differences_of_the_devices_own_bound():
    """three entries each of the inner q_mu, Z and lengthscale of a two-inner-layer model; the bar from two step sizes, as on the CPU:
    4 |fd(h) - fd(h / 2)| + 1e-9 |bound| / h.  Independent of the oracle."""
    c = T.Case("fd", 70, 17, (3, 3, 3), ard=True, seed=12)
    model = c.collapsed_model()
    bound, pairs, _ = model.compute_log_likelihood_gradients(zs=c.zs, inner=True)
    grads = {id(p): g for p, g in pairs}
    low = model.layers[0]
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    rng = np.random.default_rng(5)
    h = 1e-4

    def fd(p, idx, step):
        base = p.value.copy()
        vals = []
        for sign in (1.0, -1.0):
            v = base.copy()
            v[idx] += sign * step
            p.assign(v)
            vals.append(model.compute_log_likelihood(zs=c.zs))
        p.assign(base)
        return (vals[0] - vals[1]) / (2.0 * step)

    for p in (low.q_mu, low.feature.Z, split_kernel(low.kern)[0].lengthscales):
        for _ in range(3):
            idx = tuple(int(rng.integers(0, n)) for n in p.shape)
            f1, f2 = fd(p, idx, h), fd(p, idx, h / 2)
            bar = 4.0 * abs(f1 - f2) + 1e-9 * abs(bound) / h
            print(idx, grads[id(p)][idx], f2, bar)
            assert abs(grads[id(p)][idx] - f2) <= bar


def test_lbfgs_over_all_layers_beats_the_fit_of_the_collapsed_layer_alone():
    from doubly_stochastic_dgp.training import ScipyOptimizer
    fits = {}
    for inner in (True, False):
        c = T.Case("fit", 40, 6, (2, 2), seed=21)
        model = c.collapsed_model()
        start = model.compute_log_likelihood()
        q0 = model.layers[0].q_mu.value.copy()
        ScipyOptimizer().minimize(model, maxiter=30, inner=inner)
        fits[inner] = (start, model.compute_log_likelihood(), q0, model, c)
    (s1, e1, q0, model, c), (s0, e0, _, _, _) = fits[True], fits[False]
    print(f"start {s1!r}; after 30 iterations over all layers {e1!r}, over the collapsed layer alone {e0!r}")
    assert s1 == s0 and e1 >= s1 and e0 >= s0 and e1 >= e0
    assert not np.array_equal(model.layers[0].q_mu.value, q0)
    assert np.array_equal(fits[False][3].layers[0].q_mu.value, q0)
    # the DGP the inner layer is shared with sees the new values, on the host and in its own engine
    assert c.dgp.layers[0] is model.layers[0]
    Fm = c.dgp.propagate(c.X, S=1, zs=[np.zeros((1, 40, 2)), np.zeros((1, 40, 1))])[1][0]
    mean, _ = model.inner_engine().layer_conditional(0, c.X)
    assert_allclose(Fm[0], mean.cpu().numpy(), rtol=1e-9, atol=1e-10)


def test_collapsed_adam_first_step_determinism_and_the_likelihood_variance():
    from doubly_stochastic_dgp.training import CollapsedAdamOptimizer
    lr = 1e-3

    def build():
        c = T.Case("adam", 40, 6, (2, 2), seed=31)
        return c.collapsed_model()

    model = build()
    _, pairs, _ = model.compute_log_likelihood_gradients(inner=True)
    grads = {id(p): g for p, g in pairs}
    low, top = model.layers[0], model.layers[-1]
    before = {id(p): p.value.copy() for p in (low.q_mu, top.feature.Z)}
    CollapsedAdamOptimizer(lr).minimize(model, maxiter=1)
    for p in (low.q_mu, top.feature.Z):
        # first Adam step on an unconstrained entry, towards larger bound: lr_1 m / (sqrt(v) + eps) with m = (1 - b1) g,
        # v = (1 - b2) g^2, lr_1 = lr sqrt(1 - b2) / (1 - b1), that is lr g / (|g| + eps / sqrt(1 - b2)) = lr sign(g) up to epsilon
        g = grads[id(p)]
        step = p.value - before[id(p)]
        assert_allclose(step, lr * g / (np.abs(g) + 1e-8 / np.sqrt(1.0 - 0.999)), rtol=1e-9, atol=1e-14)
    CollapsedAdamOptimizer(lr).minimize(model, maxiter=4)
    twin = build()
    CollapsedAdamOptimizer(lr).minimize(twin, maxiter=5)
    for p, q in zip(list(model.inner_parameters()) + [top.feature.Z, model.likelihood.likelihood.variance],
                    list(twin.inner_parameters()) + [twin.layers[-1].feature.Z, twin.likelihood.likelihood.variance]):
        assert np.array_equal(_bits(p.value), _bits(q.value))
    eng = model.inner_engine()
    from doubly_stochastic_dgp.gpflow_compat import positive_forward
    off = eng.desc.off_lik_var
    eng.ctx.sync()
    on_device = float(positive_forward(eng.theta.cpu().numpy()[off]))
    assert_allclose(on_device, float(model.likelihood.likelihood.variance.value), rtol=1e-14)
