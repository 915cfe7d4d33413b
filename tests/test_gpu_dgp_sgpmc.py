"""-m gpu: model_zoo.DGP_SGPMC, the sampled deep model over SGPMC layers, through its public interface.

1. The tie to the existing engine, the reference's own trick (tests/test_zoo_models.py:99-101): a `DGP` with white=True, the same q_mu,
   q_sqrt = 1e-12 I and the same zs is the same model up to 1e-24 |a|^2 in the variances; its predict_all_layers are DGP_SGPMC's at
   rtol 1e-9, the bar the full-size fixtures hold the engine to.
2. The model's gradients against central differences of the device's own log density under fix_draws.
3. Minibatch scaling: the data term carries num_data / N, the prior is counted once; the minibatches are the rows Minibatch deals.
4. predict_density and evaluate over a run of T = 3 kept states equal the host reduction of the stacked components."""
import numpy as np
import pytest

from tests import sgpmc_stack_cases as KC

pytestmark = pytest.mark.gpu


def _small_model(num_data=None, minibatch_size=None, S=2, N=24, seed=0, lik=None):
    from doubly_stochastic_dgp import gpflow_compat as G
    from doubly_stochastic_dgp.layers import SGPMC_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_SGPMC
    rng = np.random.default_rng(seed)
    D, M = 2, 6
    X = rng.standard_normal((N, D))
    Y = np.sin(X[:, :1]) + 0.1 * rng.standard_normal((N, 1))
    Z = rng.standard_normal((M, D))
    k0 = G.RBF(D, variance=1.2, lengthscales=[1.1, 1.6], ARD=True) + G.White(D, variance=0.05)
    k1 = G.Matern52(D, variance=0.9, lengthscales=1.4)
    layers = [SGPMC_Layer(k0, Z, D, G.Identity(), white=True), SGPMC_Layer(k1, Z + 0.1, 1, G.Zero(), white=False)]
    for layer in layers:
        layer.q_mu = 0.7 * rng.standard_normal(layer.q_mu.shape)
    model = DGP_SGPMC(X, Y, G.Gaussian(0.2) if lik is None else lik, layers, minibatch_size=minibatch_size, num_samples=S, num_data=num_data)
    return model, X, Y


def test_a_dgp_with_a_vanishing_q_sqrt_is_the_same_model():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.layers import SGPMC_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_SGPMC
    rng = np.random.default_rng(3)
    N, D, M, S, Ns = 40, 3, 12, 4, 70
    X, Y, Xs = rng.standard_normal((N, D)), rng.standard_normal((N, 1)), rng.standard_normal((Ns, D))
    Z = X[:M].copy()
    dgp = DGP(X, Y, Z, [RBF(D, lengthscales=1.3), RBF(D, variance=0.8, lengthscales=1.7), RBF(D, lengthscales=2.0)], Gaussian(0.1), white=True,
              num_samples=S)
    mine = []
    for layer in dgp.layers:
        q = rng.standard_normal(layer.q_mu.shape)
        layer.q_mu = q
        layer.q_sqrt = np.tile(1e-12 * np.eye(M)[None], [layer.num_outputs, 1, 1])
        low = SGPMC_Layer(layer.kern, layer.feature.Z.value, layer.num_outputs, layer.mean_function, white=True)
        low.q_mu = q
        mine.append(low)
    model = DGP_SGPMC(X, Y, Gaussian(0.1), mine, num_samples=S)
    zs = [rng.standard_normal((S, Ns, layer.num_outputs)) for layer in dgp.layers]
    Fs0, Fm0, Fv0 = dgp.propagate(Xs, S=S, zs=zs)
    Fs1, Fm1, Fv1 = model.propagate(Xs, S=S, zs=zs)
    L = len(dgp.layers)
    for l in range(L):
        pairs = [("Fmean", Fm0[l], Fm1[l]), ("Fvar", Fv0[l], Fv1[l])] + ([("F", Fs0[l], Fs1[l])] if l + 1 < L else [])
        for k, a, b in pairs:
            assert a.shape == b.shape, (l, k)
            err = float(np.max(np.abs(a - b) / (np.abs(a) + 1e-300)))
            print("layer %d %s: max relative difference %.3g" % (l, k, err))
            np.testing.assert_allclose(b, a, rtol=1e-9, atol=0.0, err_msg="%d %s" % (l, k))
    a, b = dgp.predict_all_layers(Xs, 1), model.predict_all_layers(Xs, 1)
    assert [x.shape for part in a for x in part] == [x.shape for part in b for x in part]
    # the last layer is not sampled here (dgp.py:78-90 reads its mean and variance only): its F is its mean
    assert np.array_equal(Fs1[-1], Fm1[-1])


def test_gradients_match_central_differences_of_the_devices_own_log_density():
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    model, X, Y = _small_model(num_data=60)
    with KC.jitter(1e-3):
        model.fix_draws(11)
        value, pairs = model.compute_log_density_gradients(X, Y)
        assert model.compute_log_density(X, Y) == value               # one function under pinned draws
        h = 1e-5
        for p, g in pairs:
            assert g.shape == p.shape and np.all(np.isfinite(g))
            base = p.value.copy()
            idx = tuple(s - 1 for s in base.shape)
            for sign, store in ((1, "up"), (-1, "down")):
                v = base.copy()
                v[idx] += sign * h
                p.assign(v)
                if sign == 1:
                    up = model.compute_log_density(X, Y)
                else:
                    down = model.compute_log_density(X, Y)
            p.assign(base)
            fd = (up - down) / (2 * h)
            print("%s%s: gradient %.10g, central difference %.10g" % (type(p).__name__, base.shape, float(g[idx]), fd))
            assert abs(float(g[idx]) - fd) <= 2e-6 * max(1.0, abs(fd)), (base.shape, float(g[idx]), fd)
        assert len(pairs) == 10 and pairs[-1][0] is model.likelihood.likelihood.variance
        assert pairs[4][0] is split_kernel(model.layers[0].kern)[1].variance
        model.fix_draws(None)
        assert model.compute_log_density(X, Y) != model.compute_log_density(X, Y)      # fresh draws again


def test_minibatch_scaling_and_the_prior_counted_once():
    from doubly_stochastic_dgp.dgp import Minibatch
    N, m = 24, 8
    full, X, Y = _small_model()
    mb, _, _ = _small_model(minibatch_size=m)
    one, _, _ = _small_model(num_data=m)
    rng = np.random.default_rng(4)
    zs = [rng.standard_normal((2, m, 2))]
    Xb, Yb = X[3:3 + m], Y[3:3 + m]
    with KC.jitter(1e-3):
        a, b = mb.compute_log_likelihood(Xb, Yb, zs=zs), one.compute_log_likelihood(Xb, Yb, zs=zs)
        assert abs(a - (N / m) * b) <= 1e-13 * abs(a)
        da, db = mb.compute_log_density(Xb, Yb, zs=zs), one.compute_log_density(Xb, Yb, zs=zs)
        prior = mb.compute_log_prior()
        assert abs((da - a) - prior) <= 1e-12 * abs(da) and abs((db - b) - prior) <= 1e-12 * abs(db)
        # no X: the next minibatch, the rows Minibatch(N, m, seed=0) deals, in its order
        deal = Minibatch(N, m, seed=0)
        mb.fix_draws(5)
        for _ in range(4):                                       # past an epoch boundary
            idx = deal.next_indices()
            got = mb.compute_log_density()
            want = mb.compute_log_density(X[idx], Y[idx])
            assert got == want
        # the full model takes every row
        full.fix_draws(5)
        assert full.compute_log_density() == full.compute_log_density(X, Y)


def test_scores_over_a_run_equal_the_host_reduction_of_the_stacked_components():
    from doubly_stochastic_dgp import training
    model, X, Y = _small_model(minibatch_size=8)
    rng = np.random.default_rng(6)
    Ns, S, T = 30, 3, 3
    Xs = rng.standard_normal((Ns, 2))
    Ys = np.sin(Xs[:, :1]) + 0.1 * rng.standard_normal((Ns, 1))
    with KC.jitter(1e-3):
        run = training.SGHMC(1e-4, 0.1).sample(model, T, thin=2, burn=1, seed=2)
        assert run["samples"]["q_mu0"].shape == (T, 6, 2) and run["samples"]["q_mu1"].shape == (T, 6, 1) and run["logprobs"].shape == (T,)
        assert np.array_equal(model.layers[0].q_mu.value, run["samples"]["q_mu0"][-1])      # left at the last state
        assert not np.array_equal(run["samples"]["q_mu0"][0], run["samples"]["q_mu0"][-1])
        model.fix_draws(9)
        # the stacked components on the host: every kept state set in turn
        means, vars_ = [], []
        for t in range(T):
            for l in (0, 1):
                model.layers[l].q_mu = run["samples"]["q_mu%d" % l][t]
            m, v = model.predict_f(Xs, S)
            means.append(m), vars_.append(v)
        mean, var = np.concatenate(means, 0), np.concatenate(vars_, 0)                      # (T S, Ns, 1)
        s2 = float(model.likelihood.likelihood.variance.value)
        logp = -0.5 * np.log(2 * np.pi * (var + s2)) - 0.5 * (Ys[None] - mean) ** 2 / (var + s2)
        mx = logp.max(0)
        want = mx + np.log(np.exp(logp - mx).sum(0)) - np.log(T * S)
        got = model.predict_density(Xs, Ys, S, run=run)
        assert got.shape == (Ns, 1)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
        ev = model.evaluate(Xs, Ys, S, run=run, return_rows=True)
        mhat = mean.mean(0)
        assert ev["n"] == Ns and abs(ev["log_density"] - want.mean()) <= 1e-12 * abs(want.mean())
        assert abs(ev["rmse"] - np.sqrt(np.mean((Ys - mhat) ** 2))) <= 1e-12
        np.testing.assert_allclose(ev["rows"][:, :, 0], mhat, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ev["rows"][:, :, 1], (var + s2 + mean ** 2).mean(0) - mhat ** 2, rtol=1e-10, atol=1e-13)
        pm, pv = model.predict_y_samples(Xs, S, run)
        assert pm.shape == (T * S, Ns, 1)
        np.testing.assert_allclose(pm, mean, rtol=0, atol=0)
        np.testing.assert_allclose(pv, var + s2, rtol=1e-15)
        # the other mixture scorers take the same components
        q = model.predict_quantiles(Xs, S, probs=(0.1, 0.5, 0.9), run=run)
        assert q.shape == (Ns, 1, 3) and np.all(q[:, :, 0] < q[:, :, 1]) and np.all(q[:, :, 1] < q[:, :, 2])
        cal = model.calibration(Xs, Ys, S, run=run)
        assert cal["n"] == Ns and cal["crps"] > 0.0 and cal["pit_le"].shape == (7, 1)
        # without a run: the S components of the current state
        ev1 = model.evaluate(Xs, Ys, S)
        m1, v1 = model.predict_f(Xs, S)
        assert abs(ev1["rmse"] - np.sqrt(np.mean((Ys - m1.mean(0)) ** 2))) <= 1e-12


def test_classification_report_over_a_run():
    from doubly_stochastic_dgp import training
    from doubly_stochastic_dgp.gpflow_compat import Bernoulli
    model, X, Y = _small_model(lik=Bernoulli())
    Yb = (Y > 0).astype(np.float64)
    model.Y_data = Yb
    with KC.jitter(1e-3):
        run = training.SGHMC(1e-4, 0.1).sample(model, 2, seed=1)
        model.fix_draws(3)
        rep = model.classification_report(X, Yb, 2, bins=5, run=run, return_rows=True)
        assert rep["n"] == X.shape[0] and rep["confusion"].sum() == X.shape[0] and 0.0 <= rep["error_rate"] <= 1.0
        pm, _ = model.predict_y_samples(X, 2, run)
        np.testing.assert_allclose(rep["probs"], pm.mean(0), rtol=1e-12, atol=1e-14)


def test_test_sets_go_through_in_row_batches_that_fit_the_scratch():
    """With a scratch budget that holds a few rows only, propagate walks the test set in row batches (the given draws cut the same way)
    and returns what one batch returns; predict_y, predict_density and E_log_p_Y are the likelihood's functions of predict_f."""
    model, X, Y = _small_model()
    rng = np.random.default_rng(8)
    Ns, S = 53, 2
    Xs = rng.standard_normal((Ns, 2))
    Ys = rng.standard_normal((Ns, 1))
    zs = [rng.standard_normal((S, Ns, 2)), None]
    with KC.jitter(1e-3):
        whole = model.propagate(Xs, S=S, zs=zs)
        ctx = model._context()
        assert model._row_batch(ctx, Ns, S) == Ns
        model.scratch_budget = model._scratch_bytes(ctx, model._stack_desc(ctx)[0], 10, S, False)
        nb = model._row_batch(ctx, Ns, S)
        assert 1 <= nb <= 10
        cut = model.propagate(Xs, S=S, zs=zs)
        for a, b in zip(whole, cut):
            for x, y in zip(a, b):
                assert x.shape == y.shape
                np.testing.assert_allclose(y, x, rtol=1e-12, atol=1e-14)
        model.fix_draws(2)
        m, v = model.predict_f(Xs, S)
        assert m.shape == (S, Ns, 1) and v.shape == (S, Ns, 1)
        s2 = float(model.likelihood.likelihood.variance.value)
        pm, pv = model.predict_y(Xs, S)
        np.testing.assert_allclose(pm, m, rtol=0, atol=0)
        np.testing.assert_allclose(pv, v + s2, rtol=1e-15)
        logp = -0.5 * np.log(2 * np.pi * (v + s2)) - 0.5 * (Ys[None] - m) ** 2 / (v + s2)
        want = np.log(np.exp(logp - logp.max(0)).sum(0)) + logp.max(0) - np.log(S)
        np.testing.assert_allclose(model.predict_density(Xs, Ys, S), want, rtol=1e-12, atol=1e-12)
        e = model.E_log_p_Y(Xs, Ys)                              # the mean over num_samples = 2 components
        ve = -0.5 * np.log(2 * np.pi * s2) - 0.5 * ((Ys[None] - m) ** 2 + v) / s2
        np.testing.assert_allclose(e, ve.mean(0), rtol=1e-12, atol=1e-12)
