"""-m gpu: the engine's vector-Jacobian product (dsdgp_model_forward_saved + dsdgp_model_backward_adjoints; Engine.forward_saved /
backward_adjoints).  For seeded random adjoints dmean, dvar of the last layer's mean and variance and fixed draws, gradient_dict() is
held to torch autograd of  sum dmean mean_L + sum dvar var_L - sum KL  through the oracle: every parameter within 1e-7 of its largest
entry (the rule of tests/test_gpu_parity.py), the value -sum KL at rtol 1e-9, the likelihood's entry exactly +0.0.  The shapes are
the smallest that reach every hand-over of adjoints: the externally seeded layer as first layer (the S rows of an input row summed),
above a first layer, above an inner layer, the white=True ending, a Matern52 + White layer.  Then consistency with the engine's own
reverse pass, and the rules of the saved state."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import dgp_oracle as O
from oracle import model as OM
from tests.helpers import kern_spec, make_case

pytestmark = pytest.mark.gpu

#          n   M   input widths  outputs  white  first kernel                                   other kernels
CASES = {
    "a": (40, 6, (2,), 2, False, dict(kind="rbf"), {}),
    # 3 -> 2 through the PCA step-down Linear mean of init_layers_linear, then 2 -> 2; n ragged to the 16-row block, M padded to 32
    "b": (70, 17, (3, 2), 2, False, dict(kind="rbf", ard=True), dict(ard=True)),
    "c": (40, 6, (2, 2, 2), 2, False, dict(kind="rbf"), {}),
    "d": (70, 17, (3, 2), 2, True, dict(kind="rbf", ard=True), dict(ard=True)),
    "e": (40, 6, (2,), 2, False, dict(kind="matern52", white_variance=0.05), {}),
}
_BUILT = {}


def _spec(d, rng, kind="rbf", ard=False, white_variance=None):
    return kern_spec(kind, d, 1.1, (0.8 + 0.4 * rng.rand(d)) if ard else 0.9, ard, white_variance=white_variance)


def _case(name, S):
    """(X, spec, state, model, zs, dmean, dvar, reference value, reference gradients): built once per (case, S) and left unchanged"""
    if (name, S) not in _BUILT:
        n, M, widths, dout, white, first, other = CASES[name]
        rng = np.random.RandomState(sum(map(ord, name)) + S)
        X, Y = rng.randn(n, widths[0]), rng.randn(n, dout)
        Z = rng.uniform(-2.0, 2.0, (M, widths[0]))
        specs = [_spec(d, rng, **(first if i == 0 else dict(kind="rbf", **other))) for i, d in enumerate(widths)]
        spec, state, model = make_case(X, Y, Z, specs, white=white, S=S, seed=3)
        outs = list(widths[1:]) + [dout]
        zs = [rng.randn(S, n, d) for d in outs]
        dmean, dvar = rng.randn(S, n, dout), rng.randn(S, n, dout)
        _BUILT[(name, S)] = (X, spec, state, model, zs, dmean, dvar) + _oracle(spec, state, X, zs, S, dmean, dvar)
    return _BUILT[(name, S)]


def _oracle(spec, state, X, zs, S, dmean, dvar):
    import torch
    leaves = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in state.items()}
    m = OM.build(O.TH, spec, leaves, S)
    _, Fm, Fv = m.propagate(O.TH, torch.as_tensor(X), [torch.as_tensor(z) for z in zs], S=S)
    KL = sum(layer.KL(O.TH) for layer in m.layers)
    J = torch.sum(torch.as_tensor(dmean) * Fm[-1]) + torch.sum(torch.as_tensor(dvar) * Fv[-1]) - KL
    J.backward()
    g = {k: (t.grad.numpy().copy() if t.grad is not None else np.zeros(np.shape(state[k]))) for k, t in leaves.items()}
    return -float(KL.detach()), g, Fm[-1].detach().numpy(), Fv[-1].detach().numpy()


def _worst(g, gref, skip=()):
    return {k: float(np.max(np.abs(-gref[k] - g[k])) / (np.max(np.abs(gref[k])) + 1e-12)) for k in gref if k not in skip}


@pytest.mark.parametrize("name,S", [("a", 1), ("a", 3), ("b", 1), ("b", 3), ("c", 2), ("d", 1), ("d", 3), ("e", 2)])
def test_vjp_against_the_oracle(name, S):
    X, spec, state, model, zs, dmean, dvar, val, gref, mean_ref, var_ref = _case(name, S)
    eng = model.engine()
    mean, var = eng.forward_saved(X, S, zs=zs)
    out = eng.backward_adjoints(dmean, dvar)
    assert_allclose(mean.cpu().numpy(), mean_ref, rtol=1e-9, atol=1e-10)
    assert_allclose(var.cpu().numpy(), var_ref, rtol=1e-9, atol=1e-10)
    assert_allclose(out[0], val, rtol=1e-9)
    assert out[1] == 0.0 and out[3] == 0.0 and out[2] == -out[0]
    g = eng.gradient_dict()
    lik = g["lik_variance_raw"]
    assert lik == 0.0 and not np.signbit(lik)                       # no likelihood took part: exactly +0.0
    worst = _worst(g, gref, skip=("lik_variance_raw",))
    print(name, S, {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= 1e-7}
    assert not bad, f"gradient mismatch (relative to the largest entry): {bad}"


# ---------------------------------------------------------------------------------------------------------------- the engine's own pass
def _gaussian_two_layer(seed=5, S=2):
    rng = np.random.RandomState(seed)
    n, M, D = 70, 17, 3
    X, Y = rng.randn(n, D), rng.randn(n, 2)
    Z = rng.uniform(-2.0, 2.0, (M, D))
    specs = [_spec(D, rng), _spec(D, rng)]
    spec, state, model = make_case(X, Y, Z, specs, S=S, seed=seed, lik_var=0.3)
    zs = [rng.randn(S, n, D), rng.randn(S, n, 2)]
    return X, Y, model, zs, S


def test_gaussian_adjoints_reproduce_the_engines_own_reverse_pass():
    """dmean = w (Y - mean) / s2, dvar = -w / (2 s2), w = 1 / S, are the Gaussian likelihood's adjoints: fed to the vector-Jacobian
    product they must give the gradient of elbo(with_grad=True) in every entry but the likelihood variance's"""
    X, Y, model, zs, S = _gaussian_two_layer()
    eng = model.engine()
    eng.elbo(X, Y, S, zs=zs, with_grad=True)
    g_own = {k: v.copy() for k, v in eng.gradient_dict().items()}
    eng.grad.zero_()                                      # what is compared below was written by the vector-Jacobian product
    mean, var = eng.forward_saved(X, S, zs=zs)
    s2, w = 0.3, 1.0 / S
    dmean = w * (Y[None] - mean.cpu().numpy()) / s2
    dvar = np.full_like(dmean, -w / (2.0 * s2))
    eng.backward_adjoints(dmean, dvar)
    g = eng.gradient_dict()
    assert g["lik_variance_raw"] == 0.0 and g_own["lik_variance_raw"] != 0.0
    ratio = {k: float(np.max(np.abs(g[k] - g_own[k])) / np.max(np.abs(g_own[k]))) for k in g if k != "lik_variance_raw"}
    print("vjp with Gaussian adjoints against elbo(with_grad=True), relative to the largest entry:", {k: f"{v:.1e}" for k, v in ratio.items()})
    assert max(ratio.values()) <= 1e-7


def test_the_saved_pass_draws_what_propagate_draws_under_the_same_seed():
    """no explicit zs: the hidden layers' draws of forward_saved (head launch or side stream) are those of propagate under the same
    seed, so a caller may evaluate its scalar on one pass and differentiate through the other (DGP_Collapsed does)"""
    X, spec, state, model, zs, *_ = _case("c", 2)
    eng = model.engine()
    _, Fm, Fv = eng.propagate(X, 2, seed=11, want=("mean", "var"))
    mean, var = eng.forward_saved(X, 2, seed=11)
    _, Fm2, _ = eng.propagate(X, 2, seed=12, want=("mean", "var"))
    assert_allclose(mean.cpu().numpy(), Fm[-1].cpu().numpy(), rtol=1e-9, atol=1e-10)
    assert_allclose(var.cpu().numpy(), Fv[-1].cpu().numpy(), rtol=1e-9, atol=1e-10)
    assert not np.allclose(Fm2[-1].cpu().numpy(), Fm[-1].cpu().numpy(), rtol=1e-3)


# ---------------------------------------------------------------------------------------------------------------- the saved state
def _bits(d):
    return {k: np.asarray(v).copy().view(np.uint64) for k, v in d.items()}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_backward_without_or_after_losing_the_saved_pass_is_refused_and_writes_nothing():
    from doubly_stochastic_dgp._lib import DsdgpError
    X, Y, model, zs, S = _gaussian_two_layer(seed=6)
    eng = model.engine()
    rng = np.random.RandomState(0)
    dm, dv = rng.randn(S, 70, 2), rng.randn(S, 70, 2)
    with pytest.raises(DsdgpError, match="forward_saved"):
        eng.backward_adjoints(dm, dv)
    eng.elbo(X, Y, S, zs=zs, with_grad=True)
    before = _bits(eng.gradient_dict())
    for spoil in (lambda: eng.propagate(X, S, zs=zs), lambda: eng.elbo(X, Y, S, zs=zs),
                  lambda: model.layers[0].q_mu.assign(model.layers[0].q_mu.value * 1.0)):
        eng.forward_saved(X, S, zs=zs)
        spoil()
        with pytest.raises(DsdgpError, match="forward_saved"):
            eng.backward_adjoints(dm, dv)
        assert _same(before, _bits(eng.gradient_dict()))
    eng.forward_saved(X, S, zs=zs)
    eng.backward_adjoints(dm, dv)
    with pytest.raises(DsdgpError, match="forward_saved"):            # one reverse pass per forward pass
        eng.backward_adjoints(dm, dv)


def test_quadrature_weights_and_a_pruned_reverse_pass_are_refused():
    from doubly_stochastic_dgp import _lib
    X, Y, model, zs, S = _gaussian_two_layer(seed=8)
    eng = model.engine()
    rng = np.random.RandomState(2)
    dm, dv = rng.randn(S, 70, 2), rng.randn(S, 70, 2)
    eng.forward_saved(X, S, zs=zs)
    _lib.check(eng.lib.dsdgp_model_set_grad_first_layer(eng.model, 1))          # behind the wrapper's back: it would lift it
    try:
        with pytest.raises(_lib.DsdgpError, match="restricted"):
            eng.backward_adjoints(dm, dv)
    finally:
        _lib.check(eng.lib.dsdgp_model_set_grad_first_layer(eng.model, 0))
    eng.set_sample_weights(eng.ctx.to_device(np.full(S, 1.0 / S)))
    try:
        with pytest.raises(_lib.DsdgpError, match="sample weights"):
            eng.forward_saved(X, S, zs=zs)
    finally:
        eng.set_sample_weights(None)
    eng.forward_saved(X, S, zs=zs)
    assert eng.backward_adjoints(dm, dv)[3] == 0.0


def test_a_repeated_pair_a_fresh_engine_and_a_following_elbo_give_the_same_bits():
    rng = np.random.RandomState(1)
    dm, dv = rng.randn(2, 70, 2), rng.randn(2, 70, 2)

    def pair(eng, X, S, zs):
        eng.forward_saved(X, S, zs=zs)
        out = eng.backward_adjoints(dm, dv)
        return dict(_bits(eng.gradient_dict()), out=out.copy().view(np.uint64))

    X, Y, used, zs, S = _gaussian_two_layer(seed=7)
    first = pair(used.engine(), X, S, zs)
    assert _same(first, pair(used.engine(), X, S, zs))
    used.engine().elbo(X, Y, S, zs=zs, with_grad=True)                 # something else in between
    assert _same(first, pair(used.engine(), X, S, zs))
    _, _, fresh, _, _ = _gaussian_two_layer(seed=7)
    assert _same(first, pair(fresh.engine(), X, S, zs))
    # ... and the engine's own gradient evaluation after a pair is a fresh engine's
    _, _, fresh2, _, _ = _gaussian_two_layer(seed=7)
    o_fresh = fresh2.engine().elbo(X, Y, S, zs=zs, with_grad=True)
    o_used = used.engine().elbo(X, Y, S, zs=zs, with_grad=True)
    assert np.array_equal(o_fresh.view(np.uint64), o_used.view(np.uint64))
    assert _same(_bits(fresh2.engine().gradient_dict()), _bits(used.engine().gradient_dict()))
