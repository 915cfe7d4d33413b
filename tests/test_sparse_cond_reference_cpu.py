"""The reference of the sparse conditional without q_sqrt (tests/sparse_cond_reference.py) held, without a device, to three things it was
not written from: central differences of its own forward in long double, torch autograd of the same conditional in float64, and the
oracle's SVGP layer with q_sqrt = 0 (oracle/dgp_oracle.py: conditional_ND only — its KL is not read), for both values of `white`.  And
what the host mirror refuses needs no device either: the engine and a DGP holding an SGPMC_Layer, deeper and mixed DGP_Collapsed
models, a trainable Linear mean; the layer has q_sqrt = None and KL() == 0.0."""
import numpy as np
import pytest

from tests import sparse_cond_reference as SR

LD = np.longdouble
RBF, MATERN52 = 0, 1

#        kind      ard white_var white n   M  D  DO
CASES = {
    "rbf_w":  (RBF,      1, None, True,  9,  5, 2, 2),
    "rbf_u":  (RBF,      0, 0.3,  False, 11, 6, 3, 1),
    "m52_w":  (MATERN52, 0, 0.2,  True,  8,  4, 2, 3),
    "m52_u":  (MATERN52, 1, None, False, 10, 5, 3, 2),
}
JITTER = 1e-2


def _inputs(name):
    kind, ard, wv, white, n, M, D, DO = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    return dict(kind=kind, ard=bool(ard), wv=wv, white=white, Z=rng.standard_normal((M, D)), X=rng.standard_normal((n, D)),
                q_mu=rng.standard_normal((M, DO)), ls=np.sqrt(D) * rng.uniform(0.7, 1.4, D if ard else 1), variance=1.3,
                gm=rng.standard_normal((n, DO)), gv=rng.standard_normal(n))


def _J(c, dtype=LD, **over):
    a = dict(c, **over)
    return SR.functional(a["kind"], a["Z"], a["X"], a["q_mu"], a["variance"], a["ls"], a["wv"], JITTER, a["white"], a["gm"], a["gv"], dtype=dtype)


def _reverse(c, dtype=LD):
    return SR.reverse(c["kind"], c["Z"], c["X"], c["q_mu"], c["variance"], c["ls"], c["ard"], c["wv"], JITTER, c["white"], c["gm"], c["gv"],
                      dtype=dtype)


@pytest.mark.parametrize("name", list(CASES))
def test_reverse_matches_central_differences_in_long_double(name):
    """h = 1e-6 in long double: the truncation h^2 / 6 |J'''| is some 1e-12 of the gradient's scale, the rounding 2^-63 |J| / h some
    1e-13: 1e-9 (1 + |g|) holds both with room and excludes any wrong term"""
    c = _inputs(name)
    g, _ = _reverse(c)
    h = LD(1e-6)

    def fd(key, idx):
        lo, hi = (np.array(c[key], dtype=LD) for _ in range(2))
        lo[idx] -= h
        hi[idx] += h
        return (_J(c, **{key: hi}) - _J(c, **{key: lo})) / (2 * h)

    checks = [("q_mu", g["q_mu"][i], fd("q_mu", i)) for i in np.ndindex(c["q_mu"].shape)]
    checks += [("Z", g["Z"][i], fd("Z", i)) for i in np.ndindex(c["Z"].shape)]
    checks += [("X", g["X"][i], fd("X", i)) for i in list(np.ndindex(c["X"].shape))[::3]]
    checks.append(("variance", g["variance"][0], (_J(c, variance=LD(c["variance"]) + h) - _J(c, variance=LD(c["variance"]) - h)) / (2 * h)))
    if c["ard"]:
        checks += [("lengthscales", g["lengthscales"][d], fd("ls", d)) for d in range(len(c["ls"]))]
    else:
        checks.append(("lengthscales", g["lengthscales"][0], fd("ls", 0)))
    if c["wv"] is not None:
        checks.append(("diag", g["diag"][0], (_J(c, wv=LD(c["wv"]) + h) - _J(c, wv=LD(c["wv"]) - h)) / (2 * h)))
    worst = max(abs(float(want - got)) / (1.0 + abs(float(want))) for _, want, got in checks)
    print("%s: %d entries, worst |gradient - central difference| / (1 + |gradient|) = %.3g" % (name, len(checks), worst))
    for key, want, got in checks:
        assert abs(float(want - got)) <= 1e-9 * (1.0 + abs(float(want))), key


def _torch_conditional(torch, c, Z, X, q, variance, ls, wv):
    il = 1.0 / (ls if c["ard"] else ls.expand(Z.shape[1]))

    def K(A, B):
        u = (A[:, None, :] - B[None, :, :]) * il
        r2 = (u * u).sum(-1)
        if c["kind"] == RBF:
            return variance * torch.exp(-0.5 * r2)
        r = torch.sqrt(r2 + 1e-12)
        return variance * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * torch.exp(-np.sqrt(5.0) * r)

    M = Z.shape[0]
    diag = JITTER + (wv if wv is not None else 0.0)
    Lu = torch.linalg.cholesky(K(Z, Z) + diag * torch.eye(M, dtype=torch.float64))
    A = torch.linalg.solve_triangular(Lu, K(Z, X), upper=False)
    W = q if c["white"] else torch.linalg.solve_triangular(Lu, q, upper=False)
    kd = variance + (wv if wv is not None else 0.0)
    return A.T @ W, kd - (A * A).sum(0)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_reverse_match_torch_autograd_in_float64(name):
    """two float64 routes to the same numbers: 1e-9 (1 + |g|) is a thousand times what either loses at these sizes (cond(Ku) < 1e3)"""
    import torch
    c = _inputs(name)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=True)
    Z, X, q, variance, ls = t(c["Z"]), t(c["X"]), t(c["q_mu"]), t(c["variance"]), t(c["ls"])
    wv = t(c["wv"]) if c["wv"] is not None else None
    mean, var = _torch_conditional(torch, c, Z, X, q, variance, ls, wv)
    fwd, _ = SR.forward(c["kind"], c["Z"], c["X"], c["q_mu"], c["variance"], c["ls"], c["wv"], JITTER, c["white"])
    assert np.max(np.abs(mean.detach().numpy() - fwd["mean"].astype(np.float64))) <= 1e-10
    assert np.max(np.abs(var.detach().numpy() - fwd["var"].astype(np.float64))) <= 1e-10
    J = (torch.tensor(c["gm"]) * mean).sum() + (torch.tensor(c["gv"]) * var).sum()
    J.backward()
    g, _ = _reverse(c)
    got = dict(q_mu=q.grad, Z=Z.grad, X=X.grad, variance=variance.grad, lengthscales=ls.grad)
    if wv is not None:
        got["diag"] = wv.grad
    for k, v in got.items():
        want, v = np.asarray(g[k], dtype=np.float64).reshape(-1), v.numpy().reshape(-1)
        assert np.max(np.abs(want - v) / (1.0 + np.abs(want))) <= 1e-9, k


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_the_oracle_svgp_layer_with_a_zero_q_sqrt(name):
    """q_sqrt = 0 makes SK = -I (white) or -Ku of layers.py:195-201: the same conditional.  The oracle forms Ku^-1 Kuf and A^T Ku A where
    the reference keeps Lu^-1 Kuf, and expands the squared distance: two float64 routes, 1e-9 apart at most at these sizes"""
    from oracle import dgp_oracle as O
    c = _inputs(name)
    M, DO = c["q_mu"].shape
    kern = O.Kern("rbf" if c["kind"] == RBF else "matern52", c["Z"].shape[1], variance=c["variance"],
                  lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]), ARD=c["ard"], white_variance=c["wv"])
    layer = O.SVGPLayer(kern, c["Z"], c["q_mu"], np.zeros((DO, M, M)), O.MeanFn("zero"), white=c["white"], jitter=JITTER)
    mean, var = layer.conditional_ND(O.NP, c["X"])
    fwd, _ = SR.forward(c["kind"], c["Z"], c["X"], c["q_mu"], c["variance"], c["ls"], c["wv"], JITTER, c["white"], dtype=np.float64)
    assert np.max(np.abs(np.asarray(mean) - fwd["mean"])) <= 1e-9
    assert np.asarray(var).shape == (c["X"].shape[0], DO)
    assert np.max(np.abs(np.asarray(var) - fwd["var"][:, None])) <= 1e-9
    cov, _ = SR.full_cov(c["kind"], c["Z"], c["X"], c["q_mu"], c["variance"], c["ls"], c["wv"], JITTER, c["white"], dtype=np.float64)
    _, full = layer.conditional_ND(O.NP, c["X"], full_cov=True)
    assert np.max(np.abs(np.asarray(full)[:, :, 0] - cov)) <= 1e-9


def _layer(white=True, D=2, M=4, DO=2, mean=None):
    from doubly_stochastic_dgp.gpflow_compat import RBF as RBFKern, Zero
    from doubly_stochastic_dgp.layers import SGPMC_Layer
    rng = np.random.default_rng(5)
    return SGPMC_Layer(RBFKern(D, variance=1.0, lengthscales=1.0), rng.standard_normal((M, D)), DO, mean or Zero(), white=white)


def test_the_layer_has_no_q_sqrt_and_no_kl():
    layer = _layer()
    assert layer.q_sqrt is None and layer.KL() == 0.0
    assert layer.q_mu.shape == (4, 2) and np.all(layer.q_mu.value == 0.0) and layer.feature.Z.shape == (4, 2)
    assert layer.log_prior() == -0.5 * 8 * np.log(2.0 * np.pi)
    layer.q_mu = np.ones((4, 2))
    assert abs(layer.log_prior() - (-4.0 - 4.0 * np.log(2.0 * np.pi))) <= 1e-13


def test_engine_and_dgp_refuse_the_layer_naming_the_kl_tail():
    from doubly_stochastic_dgp.dgp import DGP_Base
    from doubly_stochastic_dgp.engine import Engine
    from doubly_stochastic_dgp.gpflow_compat import Gaussian
    layer = _layer()
    with pytest.raises(NotImplementedError, match="KL tail"):
        Engine([layer], Gaussian(), True)
    X, Y = np.zeros((6, 2)), np.zeros((6, 2))
    with pytest.raises(NotImplementedError, match="KL tail"):
        DGP_Base(X, Y, Gaussian(), [layer]).engine()


def test_collapsed_models_deeper_or_mixed_are_refused_saying_why():
    from doubly_stochastic_dgp.gpflow_compat import RBF as RBFKern, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer, SVGP_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    X, Y = np.zeros((6, 2)), np.zeros((6, 1))
    Z = np.random.default_rng(1).standard_normal((4, 2))
    top = lambda: SGPR_Layer(RBFKern(2), Z, 1, Zero())
    with pytest.raises(NotImplementedError, match="draws"):
        DGP_Collapsed(X, Y, Gaussian(), [_layer(), _layer(), top()])
    svgp = SVGP_Layer(RBFKern(2), Z, 2, Zero(), white=True)
    with pytest.raises(NotImplementedError, match="SVGP"):
        DGP_Collapsed(X, Y, Gaussian(), [svgp, _layer(), top()])
    model = DGP_Collapsed(X, Y, Gaussian(), [_layer(), top()])          # the supported shape: built without a device
    assert [p is q for p, q in zip(model.inner_parameters()[:2], (model.layers[0].feature.Z, model.layers[0].q_mu))] == [True, True]
    with pytest.raises(RuntimeError):
        model.inner_engine()


def test_a_trainable_linear_mean_is_refused():
    from doubly_stochastic_dgp.gpflow_compat import Linear
    layer = _layer(mean=Linear(A=np.ones((2, 2))))
    with pytest.raises(NotImplementedError, match="trainable Linear"):
        layer.conditional_ND(np.zeros((3, 2)))
    with pytest.raises(NotImplementedError, match="trainable Linear"):
        layer.conditional_vjp(np.zeros((3, 2)), np.zeros((3, 2)), X=np.zeros((3, 2)))


def test_optimisers_that_need_an_engine_refuse_the_model():
    from doubly_stochastic_dgp.gpflow_compat import RBF as RBFKern, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    from doubly_stochastic_dgp.training import CollapsedAdamOptimizer
    model = DGP_Collapsed(np.zeros((6, 2)), np.zeros((6, 1)), Gaussian(), [_layer(), SGPR_Layer(RBFKern(2), np.eye(2), 1, Zero())])
    with pytest.raises(NotImplementedError, match="SGPMC_Layer"):
        CollapsedAdamOptimizer().minimize(model, maxiter=1)
