"""CPU: the yardstick of the collapsed model's training tests (tests/collapsed_train_reference.py) held to the float64 restatement of
the reference's bound (tests/collapsed_reference.collapsed) and to central differences of itself; the two new entry points in the
header, the symbol list and the library; the host side of ScipyOptimizer(inner=True) on a stand-in objective; the refusals."""
import ctypes
import os

import numpy as np
import pytest

from oracle import dgp_oracle as O
from oracle import model as OM
from tests import collapsed_reference as CR
from tests import collapsed_train_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("name", ["two", "three", "white"])
def test_the_torch_bound_is_the_float64_bound_of_the_collapsed_reference(name):
    c = T.case(name)
    val, _, _, mu, s = T.reference(name)
    top = c.top
    ref = CR.collapsed(mu, s, top["Z"], top["variance"], top["lengthscales"], c.Y, top["lik_variance"], T.JITTER, dtype=np.float64)
    KL = sum(float(layer.KL(O.NP)) for layer in OM.build(O.NP, c.spec, c.state).layers)
    rel = abs(val - (float(ref["bound"]) - KL)) / abs(val)
    print(f"{name}: torch {val!r}, written-out float64 {float(ref['bound']) - KL!r}, relative difference {rel:.2e}")
    # measured at the first run: 0 in all three cases — the two float64 orders of the same operations gave the same double.  A
    # difference of 0 is "below the resolution of the measurement", one unit in the last place of the bound (2.2e-16 relative), and
    # that resolution is the measured figure the bar is ten times of
    assert rel <= 2.2e-15


def _fd(c, key, idx, h):
    vals = []
    for sign in (1.0, -1.0):
        st = {k: np.array(v, dtype=np.float64) for k, v in c.state.items()}
        st[key][idx] += sign * h
        vals.append(c.evaluate(state=st, grad=False)[0])
    return (vals[0] - vals[1]) / (2.0 * h)


@pytest.mark.parametrize("name", ["two", "three", "white"])
def test_the_autograd_gradients_agree_with_central_differences(name):
    """a handful of entries of every inner parameter; the bar comes from the differences themselves: the truncation error of fd(h) is
    about 4/3 |fd(h) - fd(h / 2)|, and the rounding of two bounds enters as 1e-9 |bound| / h at most (the bound is good to far better
    than 1e-9)"""
    c = T.case(name)
    val, g, _, _, _ = T.reference(name)
    rng = np.random.default_rng(7)
    h = 1e-4
    worst = {}
    for key, arr in c.state.items():
        if key == "lik_variance_raw":
            continue
        arr = np.asarray(arr)
        for _ in range(3 if arr.size > 1 else 1):
            idx = tuple(int(rng.integers(0, n)) for n in arr.shape)
            if key.endswith("q_sqrt") and idx[2] > idx[1]:
                idx = (idx[0], idx[2], idx[1])                     # the free variable is the lower triangle
            f1, f2 = _fd(c, key, idx, h), _fd(c, key, idx, h / 2)
            bar = 4.0 * abs(f1 - f2) + 1e-9 * abs(val) / h
            err = abs(g[key][idx] - f2)
            worst[key] = max(worst.get(key, 0.0), err / bar)
            assert err <= bar, (key, idx, g[key][idx], f2, bar)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------------------- the public surface
def test_the_entry_points_are_declared_listed_and_built():
    from doubly_stochastic_dgp import _lib
    with open(os.path.join(ROOT, "include", "dsdgp.h")) as f:
        header = f.read()
    assert "int dsdgp_model_forward_saved(dsdgp_model* m, const double* X, int64_t n, int32_t S" in header
    assert "int dsdgp_model_backward_adjoints(dsdgp_model* m, const double* dmean, const double* dvar, double kl_weight, double* out)" in header
    lib = ctypes.CDLL(_lib.lib_path())
    for name in ("dsdgp_model_forward_saved", "dsdgp_model_backward_adjoints"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


# ---------------------------------------------------------------------------------------------------------------- the optimiser's host side
def _stand_in():
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, White, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer, SVGP_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed

    class StandIn(DGP_Collapsed):
        """F = -sum (theta - target)^2 over every parameter of the model (0.5 for a positive one, else 0.25 — below the diagonal of a
        q_sqrt, 0 above it), with the gradients of the call's own list of parameters"""

        def compute_log_likelihood_gradients(self, zs=None, inner=False):
            top, lik = self.layers[-1], self.likelihood.likelihood
            params = [top.feature.Z, top.kern.variance, top.kern.lengthscales, lik.variance]
            everything = params + self.inner_parameters()
            target = lambda p: 0.5 if p.transform == "positive" else np.tril(np.full(p.shape, 0.25)) if p.transform == "tril" else 0.25
            bound = -sum(float(np.sum((p.value - target(p)) ** 2)) for p in everything if p.trainable)
            if inner:
                params = params + [p for p in self.inner_parameters() if p.trainable]
            return bound, [(p, -2.0 * (p.value - target(p))) for p in params], {}

    rng = np.random.RandomState(4)
    X, Y = rng.randn(20, 2), rng.randn(20, 1)
    low = SVGP_Layer(RBF(2, lengthscales=1.5) + White(2, variance=0.2), X[:4].copy(), 2, Zero())
    low.q_sqrt = np.tril(0.1 * rng.randn(2, 4, 4)) + np.eye(4)[None]
    low.q_mu = rng.randn(4, 2)
    top = SGPR_Layer(RBF(2, lengthscales=2.0), X[:5].copy(), 1, Zero())
    return StandIn(X, Y, Gaussian(variance=1.0), [low, top]), low, top


def test_scipy_optimizer_inner_packs_assigns_and_leaves_alone_what_it_should():
    from doubly_stochastic_dgp.training import ScipyOptimizer
    model, low, top = _stand_in()
    low.kern.split()[0].lengthscales.set_trainable(False)
    keep = low.kern.split()[0].lengthscales.value.copy()
    res = ScipyOptimizer(tol=1e-14).minimize(model, maxiter=500, inner=True)
    # Z (5 x 2), two positives and the noise | Z (4 x 2), q_mu (4 x 2), the lower triangles of q_sqrt (2 x 10), variance, White variance
    assert res.x.size == (10 + 3) + (8 + 8 + 20 + 1 + 1)
    assert res.success
    for p in [top.feature.Z, low.feature.Z, low.q_mu]:
        assert np.allclose(p.value, 0.25, atol=1e-5)
    for p in [top.kern.variance, top.kern.lengthscales, model.likelihood.likelihood.variance, low.kern.split()[0].variance,
              low.kern.split()[1].variance]:
        assert np.allclose(p.value, 0.5, atol=1e-5)
    q = low.q_sqrt.value
    assert np.array_equal(np.triu(q, 1), np.zeros_like(q)) and np.allclose(q, np.tril(np.full(q.shape, 0.25)), atol=1e-5)
    got = low.kern.split()[0].lengthscales.value
    assert np.array_equal(got.view(np.uint64), keep.view(np.uint64))               # not trainable: its bits stay


def test_scipy_optimizer_without_inner_moves_only_the_four():
    from doubly_stochastic_dgp.training import ScipyOptimizer
    model, low, top = _stand_in()
    before = [p.value.copy() for p in model.inner_parameters()]
    res = ScipyOptimizer(tol=1e-14).minimize(model, maxiter=500)
    assert res.x.size == 10 + 3 and np.allclose(top.feature.Z.value, 0.25, atol=1e-5)
    for p, b in zip(model.inner_parameters(), before):
        assert np.array_equal(p.value.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_inner_gradients_refuse_a_last_inner_layer_that_propagates_inputs():
    model, low, _ = _stand_in()
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    object.__setattr__(low, "input_prop_dim", 1)
    with pytest.raises(NotImplementedError, match="input_prop_dim"):
        DGP_Collapsed.compute_log_likelihood_gradients(model, inner=True)


def test_a_two_layer_collapsed_model_keeps_refusing_the_minibatch_optimisers():
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    from doubly_stochastic_dgp.training import AdamOptimizer, NatGradOptimizer
    model = T.case("two").collapsed_model()
    assert len(model.layers) == 2 and DGP_Collapsed.supports_gradients is False
    with pytest.raises(NotImplementedError, match="reverse pass"):
        model.train_step(0.01)
    with pytest.raises(NotImplementedError, match="reverse pass"):
        AdamOptimizer(0.01).minimize(model, maxiter=1)
    with pytest.raises(NotImplementedError, match="reverse pass"):
        NatGradOptimizer(1.0).minimize(model, var_list=[])
    with pytest.raises(NotImplementedError, match="reverse pass"):
        model._build_likelihood(with_grad=True)
