"""-m gpu: dsdgp_sghmc_step (csrc/sgpmc_stack.hip) and training.SGHMC.

One step against the long-double formula on the noise dsdgp_randn returns: theta' = theta + v, v' = (1 - alpha) v + eta g +
sqrt(2 alpha eta) xi, every entry within 4 eps x the sum of the magnitudes it adds (eps = 2^-52).  With alpha = 0 the step is plain
momentum and xi is not read.  A run replays from its seed bit for bit, another seed gives other bits, and a refused step — by the
library, or by a factorisation that fails at the new position — leaves position and momentum as they were."""
import ctypes as C

import numpy as np
import pytest

from tests import sgpmc_stack_cases as KC

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BAD_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _step(ctx, theta, v, g, xi, alpha, eta):
    t, m = ctx.to_device(theta), ctx.to_device(v)
    gd = ctx.to_device(g)
    rc = ctx.lib.dsdgp_sghmc_step(ctx.handle, theta.size, _p(t), _p(m), _p(gd), _p(xi), alpha, eta)
    ctx.sync()
    return rc, t.cpu().numpy(), m.cpu().numpy()


@pytest.mark.parametrize("count", (1, 255, 257, 1000))
def test_one_step_against_the_long_double_formula(ctx, count):
    LD = np.longdouble
    rng = np.random.default_rng(count)
    theta, v, g = rng.standard_normal(count), 0.1 * rng.standard_normal(count), 30.0 * rng.standard_normal(count)
    alpha, eta = 0.05, 3e-4
    xi = ctx.empty(count)
    assert ctx.lib.dsdgp_randn(ctx.handle, C.c_uint64(17), C.c_uint64(4), count, _p(xi)) == 0
    ctx.sync()
    xh = xi.cpu().numpy()
    rc, t1, v1 = _step(ctx, theta, v, g, xi, alpha, eta)
    assert rc == 0, ctx.lib.dsdgp_last_error()
    noise = np.sqrt(LD(2.0) * LD(alpha) * LD(eta))
    terms = [(LD(1.0) - LD(alpha)) * v.astype(LD), LD(eta) * g.astype(LD), noise * xh.astype(LD)]
    want_v, mag_v = sum(terms), sum(np.abs(t) for t in terms)
    want_t, mag_t = theta.astype(LD) + v.astype(LD), np.abs(theta) + np.abs(v)
    fig_t = float(np.max(np.abs(t1 - want_t) / (4 * EPS * mag_t)))
    fig_v = float(np.max(np.abs(v1 - want_v) / (4 * EPS * mag_v)))
    print("count %d: theta %.3g, v %.3g (x 4 eps sum of magnitudes)" % (count, fig_t, fig_v))
    assert fig_t <= 1.0 and fig_v <= 1.0
    assert _same_bits(t1, theta + v)                                   # one addition: correctly rounded


def test_without_friction_the_step_is_plain_momentum_and_reads_no_noise(ctx):
    rng = np.random.default_rng(2)
    count = 300
    theta, v, g = rng.standard_normal(count), rng.standard_normal(count), rng.standard_normal(count)
    eta = 1e-3
    xi = ctx.to_device(rng.standard_normal(count))
    nan = ctx.empty(count).fill_(float("nan"))
    rc, t0, v0 = _step(ctx, theta, v, g, xi, 0.0, eta)
    rc1, t1, v1 = _step(ctx, theta, v, g, nan, 0.0, eta)
    rc2, t2, v2 = _step(ctx, theta, v, g, None, 0.0, eta)
    assert rc == 0 and rc1 == 0 and rc2 == 0
    assert _same_bits(t0, t1) and _same_bits(v0, v1) and _same_bits(t0, t2) and _same_bits(v0, v2)
    LD = np.longdouble
    want, mag = v.astype(LD) + LD(eta) * g.astype(LD), np.abs(v) + eta * np.abs(g)
    assert np.all(np.abs(v1 - want) <= 4 * EPS * mag) and _same_bits(t1, theta + v)


def test_a_step_the_library_refuses_leaves_position_and_momentum(ctx):
    rng = np.random.default_rng(3)
    theta, v, g = rng.standard_normal(50), rng.standard_normal(50), rng.standard_normal(50)
    xi = ctx.to_device(rng.standard_normal(50))
    launches = ctx.lib.dsdgp_launch_count()
    for alpha, eta, noise in ((1.5, 1e-3, xi), (-0.1, 1e-3, xi), (0.1, 0.0, xi), (0.1, -1.0, xi), (float("nan"), 1e-3, xi), (0.1, 1e-3, None)):
        rc, t1, v1 = _step(ctx, theta, v, g, noise, alpha, eta)
        assert rc == BAD_ARG and _same_bits(t1, theta) and _same_bits(v1, v), (alpha, eta)
    assert ctx.lib.dsdgp_launch_count() == launches


def _model():
    c = KC.case("student")
    return KC.model_of(c), c


def _run(seed, iters=5, patch=None):
    from doubly_stochastic_dgp import training
    model, c = _model()
    model.minibatch_size = None
    if patch is not None:
        patch(model)
    with KC.jitter(c["jitter"]):
        run = training.SGHMC(2e-4, 0.1).sample(model, iters, seed=seed)
    return model, run


def test_a_run_replays_from_its_seed_and_another_seed_gives_other_bits():
    _, a = _run(3)
    _, b = _run(3)
    _, other = _run(4)
    assert a["names"] == ["q_mu0", "q_mu1"] and a["samples"]["q_mu0"].shape == (5, 5, 1) and a["samples"]["q_mu1"].shape == (5, 16, 2)
    for k in a["samples"]:
        assert _same_bits(a["samples"][k], b["samples"][k]), k
        assert not _same_bits(a["samples"][k], other["samples"][k]), k
        assert np.all(np.isfinite(a["samples"][k]))
    assert _same_bits(a["logprobs"], b["logprobs"])
    # the states move, one step at a time
    assert not _same_bits(a["samples"]["q_mu1"][0], a["samples"]["q_mu1"][4])


def test_other_parameters_move_in_unconstrained_space():
    from doubly_stochastic_dgp import training
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    model, c = _model()
    var = split_kernel(model.layers[1].kern)[0].variance
    scale = model.likelihood.likelihood.scale
    with KC.jitter(c["jitter"]):
        run = training.SGHMC(1e-4, 0.1).sample(model, 3, var_list=[model.layers[0].q_mu, var, scale], seed=1)
    assert run["names"] == ["q_mu0", "var1", "var2"] and run["samples"]["var1"].shape == (3,) and np.all(run["samples"]["var1"] > 1e-6)
    assert np.all(run["samples"]["var2"] > 1e-6) and float(var.value) == run["samples"]["var1"][-1]
    assert not _same_bits(run["samples"]["var1"][0], run["samples"]["var1"][2])


def test_a_failed_factorisation_at_the_new_position_restores_the_previous_state():
    """The gradient at the position after the second step raises CholeskyError (injected: the sampler sees what the library raises): the
    sampler goes back to the position and the momentum before that step and evaluates the gradient there on the next minibatch, so the
    run has the bits of one whose second iteration made no move and whose later iterations start from the restored state."""
    from doubly_stochastic_dgp import _lib
    calls = {"n": 0}

    def patch(model):
        inner = model.compute_log_density_gradients

        def failing(*a, **k):
            calls["n"] += 1
            if calls["n"] == 3:                                  # the initial gradient, after step 1, after step 2
                raise _lib.CholeskyError("injected")
            return inner(*a, **k)
        object.__setattr__(model, "compute_log_density_gradients", failing)

    model, run = _run(3, iters=2, patch=patch)
    _, ref = _run(3, iters=1)
    assert calls["n"] == 4                                       # the failed one is evaluated again at the restored position
    for k in run["samples"]:
        assert _same_bits(run["samples"][k][0], ref["samples"][k][0]), k
        assert _same_bits(run["samples"][k][1], ref["samples"][k][0]), k        # the second iteration made no move
    assert _same_bits(model.layers[0].q_mu.value, ref["samples"]["q_mu0"][0])
