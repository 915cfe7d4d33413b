"""The host helpers the model classes and trainers share, without a device.

1. training.Variables — a positive Parameter, a free one and a `tril` Parameter of shape (2, 3, 3) with its mask: assign(x) followed by
   values() returns x bit for bit in the free and the masked entries; in the positive ones within the rounding of
   positive_backward o positive_forward (the bar is derived below); chain() is g * positive_slope(value) entry by entry; a variable
   without a gradient raises the ValueError that names the trainer.
2. layers.layer_parameters and what DGP_Collapsed / DGP_SGPMC build from it: the orders and keys written out here, as the docstrings of
   top_parameters, inner_parameters, _sgpmc_gradients and parameter_list state them.
3. model_zoo.stack_gradient_layout: the offsets and the total of a two-layer shape, ARD on one layer only, as literal numbers.
4. layers.prepend_input_prop equals concat_input_prop applied layer by layer; layers.propagate_layers is the loop of dgp.py:69-74."""
import numpy as np
import pytest

from doubly_stochastic_dgp.gpflow_compat import (RBF, Gaussian, Linear, Matern52, Parameter, White, Zero, positive_backward,
                                                 positive_forward, positive_slope)
from doubly_stochastic_dgp.layers import (GPR_Layer, SGPMC_Layer, SGPR_Layer, SVGP_Layer, concat_input_prop, layer_parameters,
                                          prepend_input_prop, propagate_layers)
from doubly_stochastic_dgp.model_zoo import DGP_SGPMC, DGP_Collapsed, stack_gradient_layout
from doubly_stochastic_dgp.training import Variables

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ 1. the variable helper
def _variables():
    rng = np.random.default_rng(0)
    pos = Parameter(np.array([0.3, 1.0, 2.5]), transform="positive")
    free = Parameter(rng.standard_normal((2, 2)))
    tril = Parameter(np.tril(rng.standard_normal((2, 3, 3))), transform="tril")
    mask = np.broadcast_to(np.tril(np.ones((3, 3), dtype=bool)), (2, 3, 3))
    return pos, free, tril, mask, Variables([pos, free, tril], [None, None, mask], who="Trainer")


def test_variables_assign_then_values_returns_the_vector():
    """The bar of a positive entry.  y = softplus(x) + 1e-6 is rounded a few times (logaddexp, the sum), and positive_backward first
    takes the 1e-6 off again: y' = y - 1e-6 carries an absolute error of at most 4 eps (1 + y).  x = y' + log(1 - exp(-y')) has
    dx / dy' = 1 / (1 - exp(-y')) = 1 / positive_slope(y), so that error arrives as 4 eps (1 + y) / slope, and the evaluation of the
    logarithm and the sum add at most 4 eps (|x| + |y'|) of their own.  Bar: 8 eps (1 + y + |x|) / slope (slope <= 1)."""
    pos, free, tril, mask, v = _variables()
    x = np.concatenate([np.array([-2.0, 0.1, 1.7]), np.random.default_rng(1).standard_normal(4 + 12)])
    assert [np.shape(c) for c in v.cut(x)] == [(3,), (2, 2), (12,)]
    v.assign(v.cut(x))
    got = v.flat(v.values())
    assert got.shape == x.shape
    assert np.array_equal(got[3:].view(np.uint64), x[3:].view(np.uint64))
    y = pos.value
    assert np.array_equal(y.view(np.uint64), positive_forward(x[:3]).view(np.uint64))
    bar = 8.0 * EPS * (1.0 + y + np.abs(x[:3])) / positive_slope(y)
    print("positive entries: |difference|", np.abs(got[:3] - x[:3]), "bar", bar)
    assert np.all(np.abs(got[:3] - x[:3]) <= bar)
    assert np.array_equal(free.value.ravel(), x[3:7])
    assert np.array_equal(tril.value[mask], x[7:]) and np.all(tril.value[~mask] == 0.0)
    constrained = v.constrained(v.cut(x))
    assert all(np.array_equal(c, p.value) and c is not p.value for c, p in zip(constrained, (pos, free, tril)))


def test_variables_chain_rule_and_missing_gradient():
    pos, free, tril, mask, v = _variables()
    rng = np.random.default_rng(2)
    g = [rng.standard_normal(p.shape) for p in (pos, free, tril)]
    out = v.chain([(tril, g[2]), (pos, g[0]), (free, g[1])])                    # looked up by Parameter, returned in variable order
    want = g[0] * positive_slope(pos.value)
    assert np.array_equal(out[0].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(out[1], g[1]) and np.array_equal(out[2], g[2][mask])
    assert np.array_equal(v.flat(out), np.concatenate([want, g[1].ravel(), g[2][mask]]))
    with pytest.raises(ValueError, match="Trainer: a Parameter of var_list has no gradient"):
        v.chain([(pos, g[0]), (tril, g[2])])
    unmasked = Variables([pos, free])
    assert [c.shape for c in unmasked.cut(np.zeros(7))] == [(3,), (2, 2)]
    assert np.array_equal(unmasked.values()[0], positive_backward(pos.value))


# ------------------------------------------------------------------------------------------------ 2. the parameter table
def _same(pairs, want):
    return len(pairs) == len(want) and all(p is q and k == key for (p, k), (q, key) in zip(pairs, want))


def test_layer_parameters_orders_and_keys():
    Z = np.random.default_rng(0).standard_normal((4, 2))
    plain = SVGP_Layer(RBF(2), Z, 2, Zero())
    assert _same(layer_parameters(plain), [(plain.feature.Z, "Z"), (plain.q_mu, "q_mu"), (plain.q_sqrt, "q_sqrt"),
                                           (plain.kern.variance, "variance"), (plain.kern.lengthscales, "lengthscales")])
    rbf, wk = Matern52(2, ARD=True), White(2, 0.1)
    white = SVGP_Layer(rbf + wk, Z, 2, Zero())
    assert _same(layer_parameters(white), [(white.feature.Z, "Z"), (white.q_mu, "q_mu"), (white.q_sqrt, "q_sqrt"), (rbf.variance, "variance"),
                                           (rbf.lengthscales, "lengthscales"), (wk.variance, "white_variance")])
    mf = Linear(np.ones((2, 2)))
    lin = SVGP_Layer(RBF(2), Z, 2, mf)
    want = [(lin.feature.Z, "Z"), (lin.q_mu, "q_mu"), (lin.q_sqrt, "q_sqrt"), (lin.kern.variance, "variance"),
            (lin.kern.lengthscales, "lengthscales")]
    assert _same(layer_parameters(lin), want + [(mf.A, "A"), (mf.b, "b")])
    assert _same(layer_parameters(lin, mean=False), want)
    mf.set_trainable(False)                                                     # a fixed map without a bias is not in theta
    assert _same(layer_parameters(lin), want)
    rbf, wk = RBF(2), White(2, 0.1)
    sampled = SGPMC_Layer(rbf + wk, Z, 2, Zero(), white=True)
    assert _same(layer_parameters(sampled), [(sampled.feature.Z, "Z"), (sampled.q_mu, "q_mu"), (rbf.variance, "variance"),
                                             (rbf.lengthscales, "lengthscales"), (wk.variance, "white_variance")])


def test_collapsed_models_parameter_lists():
    rng = np.random.default_rng(0)
    X, Y, Z = rng.standard_normal((6, 2)), rng.standard_normal((6, 1)), rng.standard_normal((4, 2))
    mf = Linear(np.ones((2, 2)))
    inner = [SVGP_Layer(RBF(2) + White(2, 0.1), Z, 2, mf), SVGP_Layer(RBF(2), Z, 2, Zero())]
    top = SGPR_Layer(RBF(2), Z, 1, Zero())
    model = DGP_Collapsed(X, Y, Gaussian(), inner + [top])
    lik = model.likelihood.likelihood.variance
    assert _same(model.top_parameters(), [(top.feature.Z, "Z"), (top.kern.variance, "variance"), (top.kern.lengthscales, "lengthscales"),
                                          (lik, "lik_variance")])
    stat, wk = inner[0].kern.split()
    want = [inner[0].feature.Z, inner[0].q_mu, inner[0].q_sqrt, stat.variance, stat.lengthscales, wk.variance, mf.A, mf.b,
            inner[1].feature.Z, inner[1].q_mu, inner[1].q_sqrt, inner[1].kern.variance, inner[1].kern.lengthscales]
    got = model.inner_parameters()
    assert len(got) == len(want) and all(p is q for p, q in zip(got, want))
    rbf, wk = Matern52(2), White(2, 0.2)
    dense = GPR_Layer(rbf + wk, Linear(np.ones((2, 1)), 0.5), 1)               # a biased Linear mean: in theta, and no pair of the bound's
    dense.mean_function.set_trainable(False)
    low = SGPMC_Layer(RBF(2, ARD=True) + White(2, 0.1), Z, 2, Zero(), white=True)
    model = DGP_Collapsed(X, Y, Gaussian(), [low, dense])
    assert _same(model.top_parameters(), [(rbf.variance, "variance"), (rbf.lengthscales, "lengthscales"), (wk.variance, "white_variance"),
                                          (model.likelihood.likelihood.variance, "lik_variance")])
    stat, wk = low.kern.split()
    assert _same(layer_parameters(low, mean=False), [(low.feature.Z, "Z"), (low.q_mu, "q_mu"), (stat.variance, "variance"),
                                                     (stat.lengthscales, "lengthscales"), (wk.variance, "white_variance")])
    with pytest.raises(NotImplementedError, match="a log density needs a sampled inner layer with a prior"):
        DGP_Collapsed(X, Y, Gaussian(), inner + [top]).compute_log_prior()
    assert model.compute_log_prior() == low.log_prior() == -0.5 * low.q_mu.value.size * np.log(2.0 * np.pi)


# ------------------------------------------------------------------------------------------------ 3. the stack's flat gradient
def test_stack_gradient_layout_literal_offsets():
    blocks, lik, total = stack_gradient_layout([(4, 3, 2, True), (5, 2, 1, False)])
    assert blocks[0] == {"Z": (0, (4, 3)), "q_mu": (12, (4, 2)), "variance": (20, (1,)), "lengthscales": (21, (3,)), "white_variance": (24, (1,))}
    assert blocks[1] == {"Z": (25, (5, 2)), "q_mu": (35, (5, 1)), "variance": (40, (1,)), "lengthscales": (41, (1,)), "white_variance": (42, (1,))}
    assert (lik, total) == (43, 44)


def test_split_gradient_cuts_by_the_layout():
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((6, 3)), rng.standard_normal((6, 1))
    layers = [SGPMC_Layer(RBF(3, ARD=True), rng.standard_normal((4, 3)), 2, Zero(), white=True),
              SGPMC_Layer(RBF(2) + White(2, 0.1), rng.standard_normal((5, 2)), 1, Zero(), white=True)]
    model = DGP_SGPMC(X, Y, Gaussian(), layers)
    assert model._gradient_layout()[2] == 44
    pairs = model.split_gradient(np.arange(44.0))
    assert [p is q for (p, _), (q, _, _) in zip(pairs, model.parameter_list())] == [True] * 10
    want = [np.arange(12.0).reshape(4, 3), np.arange(12.0, 20.0).reshape(4, 2), np.array(20.0), np.arange(21.0, 24.0),
            np.arange(25.0, 35.0).reshape(5, 2), np.arange(35.0, 40.0).reshape(5, 1), np.array(40.0), np.array(41.0), np.array(42.0),
            np.array(43.0)]
    assert all(g.shape == w.shape and np.array_equal(g, w) for (_, g), w in zip(pairs, want))


# ------------------------------------------------------------------------------------------------ 4. the host layer loop
class _Stub:
    def __init__(self, p, add):
        self.input_prop_dim, self.add, self.seen = p, add, []

    def sample_from_conditional(self, F, z=None, full_cov=False):
        self.seen.append((F, z, full_cov))
        return F + self.add, F + 2.0 * self.add, F + 3.0 * self.add


@pytest.mark.parametrize("p", [0, 1, 2])
def test_prepend_input_prop_is_concat_input_prop_layer_by_layer(p):
    rng = np.random.default_rng(p)
    S, N = 2, 5
    X = rng.standard_normal((S, N, 3))
    layers = [_Stub(p, 0.0), _Stub(0, 0.0), _Stub(p, 0.0)]
    given = [[rng.standard_normal((S, N, w)) for w in (2, 3, 1)] for _ in range(3)]
    Fs, Fmeans, Fvars = ([a.copy() for a in arrays] for arrays in given)
    prepend_input_prop(X, layers, Fs, Fmeans, Fvars)
    Fin = X
    for l, layer in enumerate(layers):
        want = concat_input_prop(Fin, p, given[0][l], given[1][l], given[2][l]) if layer.input_prop_dim else [g[l] for g in given]
        for got, w in zip((Fs[l], Fmeans[l], Fvars[l]), want):
            assert got.shape == w.shape and np.array_equal(got.view(np.uint64), w.view(np.uint64))
        Fin = want[0]
    if p:
        assert np.array_equal(Fs[2][:, :, :p], Fs[1][:, :, :p]) and np.all(Fvars[0][:, :, :p] == 0.0)


def test_propagate_layers_is_the_reference_loop():
    F = np.random.default_rng(0).standard_normal((2, 5, 3))
    layers, z = [_Stub(None, 1.0), _Stub(None, 10.0)], np.ones((2, 5, 3))
    Fs, Fmeans, Fvars = propagate_layers(layers, F, [None, z], full_cov=True)
    assert np.array_equal(Fs[0], F + 1.0) and np.array_equal(Fs[1], F + 11.0)
    assert np.array_equal(Fmeans[1], F + 1.0 + 20.0) and np.array_equal(Fvars[0], F + 3.0)
    assert layers[0].seen[0][1:] == (None, True) and layers[1].seen[0][1] is z and layers[1].seen[0][0] is Fs[0]
    propagate_layers(layers, F)
    assert [s.seen[-1][1:] for s in layers] == [(None, False)] * 2
