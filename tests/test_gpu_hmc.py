"""-m gpu: training.HMC on the device, on the model of tests/hmc_cases.py (N = 6, D = 3, DY = 2).  No statistical assertions: the
integrator is held to what its order implies, and a short run is replayed decision by decision through tests/hmc_reference.py in long
double, with the device's own momenta (read back with the same seed and stream).

  * reversibility: 8 leapfrog steps at eps = 0.05, the momentum negated, 8 more, return to the start within 1e-12 absolute (the float64
    numpy prototype returns to 1e-16: tests/test_hmc_reference_cpu.py);
  * second order: at the fixed trajectory length 0.4 the energy error falls by a factor in [3.5, 4.5] from eps to eps / 2, for
    eps = 0.1, 0.05, 0.025 (the reference gives 4.002, 4.001, 4.000).  4 is the integrator's order; the margin only has to exclude
    first order (2) and a broken half step;
  * replay: 5 iterations with lmin = 1, lmax = 4: the same path lengths and accept decisions (none is marginal: the CPU test holds
    |log u - (H0 - H1)| > 1e-6 on the reference), positions within 1e-9 relative;
  * a trajectory that hits a CholeskyError is a rejection and leaves the parameters where they were."""
import numpy as np
import pytest

from tests import hmc_cases as HC
from tests import hmc_reference as HR

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture()
def model():
    return HC.build_model()


def test_log_density_and_gradient_match_the_reference(model):
    d = HC.data()
    want, grad = HC.logp_grad(LD)(np.array(d["q0"], dtype=LD))
    got, pairs = model.compute_log_density_gradients()
    assert model.compute_log_density() == got
    assert abs(got - float(want)) <= 1e-10 * abs(float(want))
    assert pairs[0][0] is model.layers[0].q_mu
    assert np.max(np.abs(pairs[0][1] - grad.astype(np.float64))) <= 1e-9 * np.max(np.abs(grad.astype(np.float64)))


def test_leapfrog_is_reversible(model):
    from doubly_stochastic_dgp.training import HMC
    d = HC.data()
    q1, p1, _ = HMC.leapfrog(model, d["q0"], d["p0"], 0.05, 8)
    q2, p2, _ = HMC.leapfrog(model, q1, -p1, 0.05, 8)
    print("return error: q %.3g, p %.3g" % (np.max(np.abs(q2 - d["q0"])), np.max(np.abs(-p2 - d["p0"]))))
    assert np.max(np.abs(q2 - d["q0"])) <= 1e-12 and np.max(np.abs(-p2 - d["p0"])) <= 1e-12
    assert np.max(np.abs(q1 - d["q0"])) > 1e-2                                  # it did move
    assert np.array_equal(model.layers[0].q_mu.value, q2)                       # the parameters are left at the new position


def test_energy_error_is_second_order(model):
    from doubly_stochastic_dgp.training import HMC
    d = HC.data()
    model.layers[0].q_mu = d["q0"]
    H0 = -model.compute_log_density() + 0.5 * np.sum(d["p0"] ** 2)
    err = {}
    for eps, steps in ((0.1, 4), (0.05, 8), (0.025, 16), (0.0125, 32)):
        q, p, logp = HMC.leapfrog(model, d["q0"], d["p0"], eps, steps)
        err[eps] = abs((-logp + 0.5 * np.sum(p * p)) - H0)
    for eps in (0.1, 0.05, 0.025):
        ratio = err[eps] / err[eps / 2]
        print("energy error ratio at eps = %g: %.4f" % (eps, ratio))
        assert 3.5 <= ratio <= 4.5, (eps, ratio)


def test_a_short_run_replays_through_the_reference(model):
    from doubly_stochastic_dgp.training import HMC
    d = HC.data()
    var_list = [model.layers[0].q_mu]
    momenta = [HMC.momenta(model, var_list, HC.SEED, i)[0].cpu().numpy() for i in range(HC.ITERS)]
    out = HMC().sample(model, HC.ITERS, HC.EPS_REPLAY, lmin=HC.LMIN, lmax=HC.LMAX, seed=HC.SEED)
    run = HR.replay(HC.logp_grad(LD), np.array(d["q0"], dtype=LD), momenta, HC.EPS_REPLAY, HC.LMIN, HC.LMAX, HC.SEED)
    assert all(abs(r["margin"]) > 1e-6 for r in run)
    assert out["accepted"].tolist() == [r["accept"] for r in run]
    assert out["accept_rate"] == np.mean([r["accept"] for r in run])
    samples = out["samples"]["q_mu"]
    assert samples.shape == (HC.ITERS, HC.N, HC.D_X) and out["logprobs"].shape == (HC.ITERS,)
    for i, r in enumerate(run):
        want = r["q"].astype(np.float64)
        assert np.max(np.abs(samples[i] - want)) <= 1e-9 * np.max(np.abs(want)), i
    assert np.array_equal(model.layers[0].q_mu.value, samples[-1])              # the model is left at the last state
    # the same seed gives the same run; thinning and burn-in keep every thin-th state after the burn-in
    model.layers[0].q_mu = d["q0"]
    again = HMC().sample(model, 2, HC.EPS_REPLAY, lmin=HC.LMIN, lmax=HC.LMAX, thin=2, burn=1, seed=HC.SEED)
    assert np.array_equal(again["samples"]["q_mu"], samples[[2, 4]]) and again["accepted"].tolist() == out["accepted"].tolist()


def test_a_failed_factorisation_inside_a_trajectory_is_a_rejection(model):
    from doubly_stochastic_dgp._lib import CholeskyError
    from doubly_stochastic_dgp.training import HMC
    d = HC.data()
    inner, calls = model.compute_log_density_gradients, [0]

    def failing():
        calls[0] += 1
        if calls[0] > 1:                       # the evaluation at the start succeeds, every one inside a trajectory fails
            raise CholeskyError("Cholesky decomposition was not successful")
        return inner()

    model.compute_log_density_gradients = failing
    out = HMC().sample(model, 3, 0.1, lmin=2, lmax=2, seed=1)
    assert calls[0] == 4 and not out["accepted"].any() and out["accept_rate"] == 0.0
    assert all(np.array_equal(s, d["q0"]) for s in out["samples"]["q_mu"])
    assert np.array_equal(model.layers[0].q_mu.value, d["q0"])
