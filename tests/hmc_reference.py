"""Reference of training.HMC in numpy, at a chosen precision: the leapfrog integrator with unit mass and the accept / reject loop, on
any log density given as a function q -> (value, gradient) (tests/dense_reference.py: log_density of the two-layer dense model).  The
random numbers are the device run's own: the momenta are handed in (read back from dsdgp_randn with the same seed and stream), the path
lengths and the acceptance uniforms come from np.random.default_rng(seed), one integers(lmin, lmax + 1) and one uniform() per iteration,
in that order — so a run can be replayed decision by decision."""
import numpy as np


def leapfrog(logp_grad, q, p, eps, steps, grad=None):
    """-> (q, p, log density at q, gradient at q) after `steps` steps: a half step of the momentum, then position and momentum in turn,
    the last momentum step a half one"""
    dtype = np.asarray(q).dtype.type
    eps = dtype(eps)
    q, p = np.array(q), np.array(p)
    if grad is None:
        _, grad = logp_grad(q)
    p = p + dtype(0.5) * eps * grad
    logp = None
    for s in range(int(steps)):
        q = q + eps * p
        logp, grad = logp_grad(q)
        p = p + (eps if s + 1 < int(steps) else dtype(0.5) * eps) * grad
    return q, p, logp, grad


def energy(logp, p):
    return -logp + np.asarray(p).dtype.type(0.5) * np.sum(p * p)


def replay(logp_grad, q0, momenta, eps, lmin, lmax, seed):
    """-> one dict per iteration: steps, u, H0, H1, margin = log u - (H0 - H1), accept, q (the state after the iteration).  A
    factorisation that fails inside a trajectory (LinAlgError) is a rejection with margin = +inf."""
    rng = np.random.default_rng(seed)
    q = np.array(q0)
    logp, grad = logp_grad(q)
    out = []
    for p0 in momenta:
        steps, u = int(rng.integers(int(lmin), int(lmax) + 1)), float(rng.uniform())
        p0 = np.asarray(p0, dtype=q.dtype)
        H0 = energy(logp, p0)
        try:
            q1, p1, logp1, grad1 = leapfrog(logp_grad, q, p0, eps, steps, grad)
            H1 = energy(logp1, p1)
            margin = float(np.log(u) - (H0 - H1))
        except np.linalg.LinAlgError:
            H1, margin = None, float("inf")
        accept = margin < 0.0
        if accept:
            q, logp, grad = q1, logp1, grad1
        out.append(dict(steps=steps, u=u, H0=H0, H1=H1, margin=margin, accept=accept, q=q.copy()))
    return out
