"""Conditions on the references of the HMC tests alone (tests/hmc_reference.py on tests/dense_reference.py's log density, the model of
tests/hmc_cases.py), on the CPU: the gradient is the gradient of the value, the integrator is reversible and of second order at the
figures tests/test_gpu_hmc.py quotes, and no accept decision of the replayed run is marginal — |log u - (H0 - H1)| > 1e-6 at every
iteration, with the library's own momenta (oracle/philox.py reproduces dsdgp_randn)."""
import numpy as np

from oracle.philox import randn_reference
from tests import hmc_cases as HC
from tests import hmc_reference as HR

LD = np.longdouble


def test_gradient_is_the_gradient_of_the_log_density():
    f, d = HC.logp_grad(LD), HC.data()
    q = np.array(d["q0"], dtype=LD)
    _, g = f(q)
    h = LD(1e-5)
    for i, j in ((0, 0), (3, 1), (5, 2)):
        a, b = q.copy(), q.copy()
        a[i, j] += h
        b[i, j] -= h
        fd = (f(a)[0] - f(b)[0]) / (2 * h)
        assert abs(fd - g[i, j]) <= 1e-8 * (1.0 + abs(g[i, j])), (i, j, float(fd), float(g[i, j]))


def test_leapfrog_is_reversible_and_second_order():
    f, d = HC.logp_grad(np.float64), HC.data()
    q0, p0 = np.array(d["q0"]), np.array(d["p0"])
    q1, p1, _, _ = HR.leapfrog(f, q0, p0, 0.05, 8)
    q2, p2, _, _ = HR.leapfrog(f, q1, -p1, 0.05, 8)
    assert np.max(np.abs(q2 - q0)) <= 1e-14 and np.max(np.abs(-p2 - p0)) <= 1e-14
    fl = HC.logp_grad(LD)
    q0, p0 = q0.astype(LD), p0.astype(LD)
    H0 = HR.energy(fl(q0)[0], p0)
    err = {}
    for eps, steps in ((0.1, 4), (0.05, 8), (0.025, 16), (0.0125, 32)):
        q, p, logp, _ = HR.leapfrog(fl, q0, p0, eps, steps)
        err[eps] = abs(HR.energy(logp, p) - H0)
    for eps in (0.1, 0.05, 0.025):
        ratio = float(err[eps] / err[eps / 2])
        print("energy error ratio at eps = %g: %.4f" % (eps, ratio))
        assert 3.5 <= ratio <= 4.5, (eps, ratio)


def test_no_accept_decision_of_the_replayed_run_is_marginal():
    d = HC.data()
    momenta = [randn_reference(HC.SEED, i, HC.N * HC.D_X).reshape(HC.N, HC.D_X) for i in range(HC.ITERS)]
    run = HR.replay(HC.logp_grad(LD), np.array(d["q0"], dtype=LD), momenta, HC.EPS_REPLAY, HC.LMIN, HC.LMAX, HC.SEED)
    print([(r["steps"], r["accept"], "%.3g" % r["margin"]) for r in run])
    assert all(abs(r["margin"]) > 1e-6 for r in run)
    assert any(r["accept"] for r in run) and not all(r["accept"] for r in run)
    assert len({r["steps"] for r in run}) > 1


def test_a_failed_factorisation_is_a_rejection():
    d = HC.data()
    q0 = np.array(d["q0"])
    momenta = [randn_reference(HC.SEED, i, HC.N * HC.D_X).reshape(HC.N, HC.D_X) for i in range(2)]
    run = HR.replay(HC.logp_grad(np.float64, fail_when=lambda q: not np.array_equal(q, q0)), q0, momenta, HC.EPS_REPLAY, 1, 1, HC.SEED)
    assert not any(r["accept"] for r in run) and all(np.array_equal(r["q"], q0) for r in run)
