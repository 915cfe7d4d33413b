"""The reference of the stack of sparse sampled layers (tests/sgpmc_stack_reference.py) held to two independent derivations, the case
table (tests/sgpmc_stack_cases.py) held to the conditions its bars rest on, and the refusals of the model that need no device.

1. Central differences of the float64 twin's own log density, on entries of every gradient array (the likelihood's parameter included).
2. torch autograd of a direct restatement of the stack (kernels, Cholesky, solves, hops, closed-form Gaussian and Poisson expectations)
   on the one-layer and the three-layer case: every entry of every gradient array.  The `diag` entry is the gradient in what is added
   to Ku's diagonal (and, with a White part, to the kernel's diagonal kd): the restatement carries it as a leaf of its own.
3. In every case and every output array the float64 twin's own error against long double stays below 1e-9 of the array's largest
   magnitude, and no sampled layer has var + jitter below 1e-8 of the kernel's diagonal kd, except the one deliberate zero-variance
   row of the forward-only case, where it is exactly 0 in both precisions.
4. DGP_SGPMC refuses a layer that is no SGPMC_Layer, engine(), a trainable Linear mean; HMC, AdamOptimizer and ScipyOptimizer refuse
   the model, SGHMC any other model."""
import copy

import numpy as np
import pytest

from tests import sgpmc_stack_cases as KC
from tests import sgpmc_stack_reference as KR


# ------------------------------------------------------------------------------------------------ 1. central differences
def _perturbed(c, l, key, idx, h):
    c = copy.deepcopy(c)
    if key == "lik":
        name, p0, p1 = c["lik"]
        c["lik"] = (name, p0 + h, p1)
        return c
    y = c["layers"][l]
    if key == "variance":
        y["variance"] = y["variance"] + h
    elif key == "white_var":
        y["white_var"] = y["white_var"] + h
    else:
        a = np.array({"Z": y["Z"], "q_mu": y["q_mu"], "lengthscales": y["ls"]}[key], dtype=np.float64)
        a[idx] += h
        y[{"Z": "Z", "q_mu": "q_mu", "lengthscales": "ls"}[key]] = a
    return c


@pytest.mark.parametrize("name", ("r1", "student", "r255"))
def test_gradient_matches_central_differences(name):
    c = KC.case(name)
    g = KC.logdensity(name, np.float64)
    f = lambda cc: float(KR.logdensity(cc, np.float64, want_grad=False)["value"])
    h = 1e-5
    checks = []
    for l, y in enumerate(c["layers"]):
        checks += [(l, "Z", (y["M"] - 1, 0)), (l, "q_mu", (0, y["DO"] - 1)), (l, "variance", None), (l, "lengthscales", (len(y["ls"]) - 1,))]
        if y["white_var"] is not None:
            checks.append((l, "white_var", None))
    if c["lik"][0] in ("gaussian", "student_t"):
        checks.append((None, "lik", None))
    for l, key, idx in checks:
        fd = (f(_perturbed(c, l, key, idx, h)) - f(_perturbed(c, l, key, idx, -h))) / (2 * h)
        if key == "lik":
            got = float(g["lik"][0])
        else:
            arr = g["grads"][l][{"white_var": "diag"}.get(key, key)]
            got = float(arr[idx] if idx is not None else arr[0])
        print(name, l, key, idx, got, fd)
        assert abs(got - fd) <= 2e-6 * max(1.0, abs(fd)), (l, key, idx, got, fd)


# ------------------------------------------------------------------------------------------------ 2. torch autograd of a restatement
def _torch_stack(c):
    import torch
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=True)
    n, S, jitter = c["n"], c["S"], c["jitter"]
    leaves = []
    Xin = torch.tensor(np.tile(c["X"], (S, 1)), dtype=torch.float64)
    L = len(c["layers"])
    prior = 0.0

    def K(kind, A, B, variance, ls):
        d = (A[:, None, :] - B[None, :, :]) / ls
        r2 = (d * d).sum(-1)
        if kind == KC.RBF:
            return variance * torch.exp(-0.5 * r2)
        r = torch.sqrt(r2 + 1e-300)
        return variance * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * torch.exp(-np.sqrt(5.0) * r)

    for l, y in enumerate(c["layers"]):
        Z, q, var, ls = t(y["Z"]), t(y["q_mu"]), t(y["variance"]), t(y["ls"])
        diag = t(y["white_var"] if y["white_var"] is not None else 0.0)
        leaves.append(dict(Z=Z, q_mu=q, variance=var, lengthscales=ls, diag=diag))
        M = y["M"]
        Ku = K(y["kind"], Z, Z, var, ls) + (diag + jitter) * torch.eye(M, dtype=torch.float64)
        Lu = torch.linalg.cholesky(Ku)
        A = torch.linalg.solve_triangular(Lu, K(y["kind"], Z, Xin, var, ls), upper=False)
        W = q if y["white"] else torch.linalg.solve_triangular(Lu, q, upper=False)
        kd = var + diag if y["white_var"] is not None else var
        mean, v = A.T @ W, kd - (A * A).sum(0)
        if y["mean"] == "identity":
            mean = mean + Xin
        elif y["mean"] == "linear":
            mean = mean + Xin @ torch.tensor(y["A"]) + torch.tensor(y["b"])
        prior = prior - 0.5 * (q * q).sum() - 0.5 * q.numel() * np.log(2.0 * np.pi)
        if l + 1 < L:
            z = torch.tensor(c["zs"][l])
            Xin = torch.cat([Xin[:, :y["p"]], mean + z * torch.sqrt(v + jitter)[:, None]], 1)
    name, p0, p1 = c["lik"]
    Y = torch.tensor(np.tile(c["Y"], (S, 1)))
    lik = t(p0)
    vb = v[:, None]
    if name == "gaussian":
        ve = -0.5 * np.log(2.0 * np.pi) - 0.5 * torch.log(lik) - 0.5 * ((Y - mean) ** 2 + vb) / lik
    else:                                                                            # poisson, exp link, binsize p1
        ve = Y * mean - torch.exp(mean + 0.5 * vb) * p1 - torch.lgamma(Y + 1.0) + Y * np.log(p1)
    data = c["data_scale"] / S * ve.sum()
    value = data + prior
    value.backward()
    return float(value.detach()), float(data.detach()), float(prior.detach()), leaves, lik


@pytest.mark.parametrize("name", ("r1", "r800"))
def test_every_gradient_entry_matches_torch_autograd(name):
    c = KC.case(name)
    ref = KC.logdensity(name, np.float64)
    value, data, prior, leaves, lik = _torch_stack(c)
    assert abs(value - float(ref["value"])) <= 1e-11 * abs(value)
    assert abs(data - float(ref["data"])) <= 1e-11 * abs(data) and abs(prior - float(ref["prior"])) <= 1e-12 * abs(prior)
    for l, leaf in enumerate(leaves):
        for k, x in leaf.items():
            if k == "diag" and c["layers"][l]["white_var"] is None:
                continue              # without a White part the entry is the gradient in Ku's jitter alone: the leaf above feeds kd too
            want, got = x.grad.numpy().reshape(-1), np.asarray(ref["grads"][l][k], dtype=np.float64).reshape(-1)
            err = float(np.max(np.abs(want - got)))
            print(name, l, k, err, float(np.max(np.abs(want))))
            assert err <= 1e-9 * max(1.0, float(np.max(np.abs(want)))), (l, k, err)
    if name == "r1":
        assert abs(float(lik.grad) - float(ref["lik"][0])) <= 1e-10 * abs(float(lik.grad))
    else:
        assert float(ref["lik"][0]) == 0.0


# ------------------------------------------------------------------------------------------------ 3. the case table's conditions
@pytest.mark.parametrize("name", KC.NAMES + [KC.FORWARD_ONLY])
def test_the_case_table_meets_the_conditions_its_bars_rest_on(name):
    c = KC.case(name)
    tr, tw = KC.propagate(name), KC.propagate(name, np.float64)
    arrays = {"%s%d" % (k, l): (a, b) for k in ("F", "Fmean", "var") for l, (a, b) in enumerate(zip(tr[k], tw[k]))}
    if name != KC.FORWARD_ONLY:
        a, b = KR.flat_arrays(KC.logdensity(name)), KR.flat_arrays(KC.logdensity(name, np.float64))
        arrays.update({k: (a[k], b[k]) for k in a})
    for k, (a, b) in arrays.items():
        mag = float(np.max(np.abs(a)))
        err = float(np.max(np.abs(np.asarray(b) - a)))
        assert err <= 1e-9 * mag, (k, err, mag)
    for l, y in enumerate(c["layers"][:-1]):
        kd = y["variance"] + (y["white_var"] or 0.0)
        v = np.asarray(tr["var"][l], dtype=np.float64) + c["jitter"]
        if name == KC.FORWARD_ONLY and l == 0:
            rows = np.arange(KC.ZERO_ROW, c["n"] * c["S"], c["n"])
            assert np.all(tr["var"][l][rows] == 0.0) and np.all(tw["var"][l][rows] == 0.0)       # exactly, at both precisions
            assert np.all(tr["F"][l][rows] == tr["Fmean"][l][rows])
            v = np.delete(v, rows)
        assert np.all(v >= 1e-8 * kd), (l, float(v.min()))


def test_the_table_reaches_every_branch():
    layers = [y for name in KC.NAMES for y in KC.case(name)["layers"]]
    assert {len(KC.case(n)["layers"]) for n in KC.NAMES} == {1, 2, 3}
    assert {KC.case(n)["n"] * KC.case(n)["S"] for n in KC.NAMES} >= {1, 255, 257, 800}
    assert {y["DO"] for y in layers} >= {1, 3, 16, 17} and {y["p"] for y in layers} == {0, 2} and {y["M"] for y in layers} == {5, 16}
    assert {y["mean"] for y in layers} == {"zero", "identity", "linear"} and {y["white"] for y in layers} == {True, False}
    assert any(y["mean"] == "linear" and y["D"] == 5 and y["DO"] == 3 for y in layers)
    assert {y["kind"] for y in layers} == {KC.RBF, KC.MATERN52} and {y["ard"] for y in layers} == {True, False}
    assert any(y["white_var"] is not None for y in layers)
    assert {KC.case(n)["lik"][0] for n in KC.NAMES} == {"gaussian", "bernoulli", "poisson", "student_t", "multiclass"}
    assert {KC.case(n)["zmode"] for n in KC.NAMES} == {"given", "drawn"}


# ------------------------------------------------------------------------------------------------ 4. refusals that need no device
def _layers(D=2, M=4, mean=None):
    from doubly_stochastic_dgp.gpflow_compat import RBF, Zero
    from doubly_stochastic_dgp.layers import SGPMC_Layer
    Z = np.random.default_rng(0).standard_normal((M, D))
    return [SGPMC_Layer(RBF(D), Z, D, Zero() if mean is None else mean, white=True), SGPMC_Layer(RBF(D), Z, 1, Zero(), white=True)]


def _data(D=2, n=6):
    rng = np.random.default_rng(1)
    return rng.standard_normal((n, D)), rng.standard_normal((n, 1))


def test_the_model_refuses_what_it_does_not_run():
    from doubly_stochastic_dgp.gpflow_compat import RBF, Bernoulli, Gaussian, Linear, Zero
    from doubly_stochastic_dgp.layers import SVGP_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_SGPMC
    from doubly_stochastic_dgp import training
    X, Y = _data()
    model = DGP_SGPMC(X, Y, Gaussian(), _layers(), minibatch_size=3, num_samples=2)
    assert model.num_data == 6 and model.minibatch_size == 3 and model.num_samples == 2
    with pytest.raises(NotImplementedError, match="q_sqrt"):
        model.engine()
    with pytest.raises(NotImplementedError):
        model.train_step()
    with pytest.raises(ValueError, match="SGPMC_Layer"):
        DGP_SGPMC(X, Y, Gaussian(), [_layers()[0], SVGP_Layer(RBF(2), X[:4], 1, Zero(), white=True)])
    with pytest.raises(NotImplementedError, match="trainable Linear"):
        DGP_SGPMC(X, Y, Gaussian(), _layers(mean=Linear(np.eye(2))))
    fixed = Linear(np.eye(2))
    fixed.set_trainable(False)
    DGP_SGPMC(X, Y, Bernoulli(), _layers(mean=fixed))                  # a fixed map and any likelihood of the project are taken
    last = _layers()
    last[-1].input_prop_dim = 1
    with pytest.raises(ValueError, match="input_prop_dim"):
        DGP_SGPMC(X, Y, Gaussian(), last)
    with pytest.raises(NotImplementedError):
        training.HMC().sample(model, 2, 0.01)
    with pytest.raises(NotImplementedError):
        training.AdamOptimizer(0.01).minimize(model, maxiter=1)
    with pytest.raises(NotImplementedError):
        training.ScipyOptimizer().minimize(model, maxiter=1)
    with pytest.raises(NotImplementedError):
        training.NatGradOptimizer(0.1).minimize(model, [[model.layers[0].q_mu, model.layers[0].q_mu]])


def test_sghmc_refuses_other_models_and_bad_settings():
    from doubly_stochastic_dgp import training

    class Other:
        pass
    with pytest.raises(NotImplementedError, match="DGP_SGPMC"):
        training.SGHMC(1e-3, 0.1).sample(Other(), 2)
    for lr, fr in ((0.0, 0.1), (-1.0, 0.1), (1e-3, -0.1), (1e-3, 1.5)):
        with pytest.raises(ValueError):
            training.SGHMC(lr, fr)


def test_the_prior_and_the_parameter_list_on_the_host():
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, Poisson
    from doubly_stochastic_dgp.model_zoo import DGP_SGPMC
    X, Y = _data()
    layers = _layers()
    rng = np.random.default_rng(2)
    for layer in layers:
        layer.q_mu = rng.standard_normal(layer.q_mu.shape)
    model = DGP_SGPMC(X, Y, Gaussian(), layers)
    want = sum(-0.5 * np.sum(y.q_mu.value ** 2) - 0.5 * y.q_mu.value.size * np.log(2 * np.pi) for y in layers)
    assert abs(model.compute_log_prior() - want) <= 1e-13 * abs(want)
    keys = [(l, k) for _, l, k in model.parameter_list()]
    assert keys == [(0, "Z"), (0, "q_mu"), (0, "variance"), (0, "lengthscales"), (1, "Z"), (1, "q_mu"), (1, "variance"), (1, "lengthscales"),
                    (None, "lik")]
    assert model.parameter_list()[-1][0] is model.likelihood.likelihood.variance
    assert [(l, k) for _, l, k in DGP_SGPMC(X, np.abs(np.round(Y)), Poisson(), _layers()).parameter_list()][-1] == (1, "lengthscales")
