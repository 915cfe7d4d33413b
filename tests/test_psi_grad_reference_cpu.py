"""CPU: the yardstick of the reverse pass of the kernel expectations (tests/psi_grad_reference.py) held to three things of its own —
central differences in long double of tests/psi_reference.psi (and of tests/collapsed_reference.collapsed for the adjoints of the
collapsed bound), torch autograd in float64 through the direct form, and g_psi2 against its transpose — and the new entry point's
place in the header, the host mirror's symbol list and the built library.  The differences are O(h^2) with h = 1e-5 of the scale of
the inputs: agreement to 1e-7 of the entry's `mag` is their own accuracy."""
import ctypes
import os

import numpy as np
import pytest

from tests import collapsed_reference as CR
from tests import psi_grad_cases as GC
from tests import psi_grad_reference as R
from tests import psi_reference as P

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_CASES = ("n15", "n17", "m33", "zero")                  # without ARD, M = 1 with ARD, three tile rows, s = 0
H = LD(1e-5)


def _objective(c, mu, s, Z, v, ls):
    p0, p1, p2 = P.psi(mu, s, Z, v, ls, dtype=LD)
    return LD(c["g0"]) * p0 + np.sum(np.asarray(c["g1"], dtype=LD) * p1) + np.sum(np.asarray(c["g2"], dtype=LD) * p2)


def _central(fun, x, h=H):
    """central differences of the scalar fun over every entry of the long-double array x"""
    x = np.array(x, dtype=LD)
    out = np.zeros_like(x)
    flat, of = x.reshape(-1), out.reshape(-1)
    for k in range(flat.size):
        keep = flat[k]
        flat[k] = keep + h
        up = fun(x)
        flat[k] = keep - h
        dn = fun(x)
        flat[k] = keep
        of[k] = (up - dn) / (LD(2) * h)
    return out


def _close(got, fd, mag, rel=1e-7):
    err = np.abs(np.asarray(got) - np.asarray(fd)).astype(np.float64)
    assert np.all(err <= rel * np.asarray(mag, dtype=np.float64) + 1e-300), float(np.max(err / (np.asarray(mag, dtype=np.float64) + 1e-300)))


@pytest.mark.parametrize("name", FD_CASES)
def test_reference_matches_central_differences(name):
    c = GC.inputs(name)
    g, mag = GC.truth(name)
    mu, Z = np.asarray(c["mu"], dtype=LD), np.asarray(c["Z"], dtype=LD)
    n, D = mu.shape
    s = np.zeros((n, D), dtype=LD) if c["s"] is None else np.asarray(c["s"], dtype=LD)
    ls = np.asarray(c["ls"], dtype=LD)
    v = LD(c["variance"])
    _close(g["X_mean"], _central(lambda x: _objective(c, x, s, Z, v, ls), mu), mag["X_mean"])
    _close(g["X_var"], _central(lambda x: _objective(c, mu, x, Z, v, ls), s), mag["X_var"])
    _close(g["Z"], _central(lambda x: _objective(c, mu, s, x, v, ls), Z), mag["Z"])
    _close(g["variance"], _central(lambda x: _objective(c, mu, s, Z, x[0], ls), np.array([v])), mag["variance"])
    _close(g["lengthscales"], _central(lambda x: _objective(c, mu, s, Z, v, x), ls), mag["lengthscales"])


def _torch_objective(torch, mu, s, Z, v, ls, g0, g1, g2):
    """the direct form of tests/psi_reference.psi in torch float64"""
    l2 = ls * ls
    d1 = mu[:, None, :] - Z[None, :, :]
    a1 = l2 + s
    psi1 = v * torch.sqrt(torch.prod(l2 / a1, dim=1))[:, None] * torch.exp(-0.5 * torch.sum(d1 * d1 / a1[:, None, :], dim=2))
    dz = Z[:, None, :] - Z[None, :, :]
    e0 = torch.sum(dz * dz / (4.0 * l2), dim=2)
    a2 = l2 + 2.0 * s
    dm = (d1[:, :, None, :] + d1[:, None, :, :]) / 2.0
    e1 = torch.sum(dm * dm / a2[:, None, None, :], dim=3)
    psi2 = torch.sum(v * v * torch.sqrt(torch.prod(l2 / a2, dim=1))[:, None, None] * torch.exp(-(e0[None] + e1)), dim=0)
    return g0 * mu.shape[0] * v + torch.sum(g1 * psi1) + torch.sum(g2 * psi2)


@pytest.mark.parametrize("name", ("n15", "m33", "split", "d30", "huge_s", "offset"))
def test_reference_matches_torch_autograd(name):
    torch = pytest.importorskip("torch")
    c = GC.inputs(name)
    g = GC.float64(name)
    mag = GC.truth(name)[1]
    n, D = c["mu"].shape
    leaf = lambda a: torch.tensor(np.array(a, dtype=np.float64), requires_grad=True)
    mu, s, Z, v = leaf(c["mu"]), leaf(c["s"]), leaf(c["Z"]), leaf(c["variance"])
    lsp = leaf(c["ls"])
    ls = lsp if c["ard"] else lsp.expand(D)
    F = _torch_objective(torch, mu, s, Z, v, ls, c["g0"], torch.tensor(np.array(c["g1"])), torch.tensor(np.array(c["g2"])))
    F.backward()
    for key, t in (("X_mean", mu), ("X_var", s), ("Z", Z), ("variance", v), ("lengthscales", lsp)):
        _close(g[key], t.grad.numpy().reshape(np.shape(g[key])), mag[key], rel=64 * 2.0 ** -50)


def test_g_psi2_and_its_transpose_give_the_same_result():
    c = GC.inputs("m33")
    a = list(GC.args(c))
    g = R.psi_grad(*a, dtype=np.float64)[0]
    a[8] = np.ascontiguousarray(c["g2"].T)
    gt = R.psi_grad(*a, dtype=np.float64)[0]
    for k in R.KEYS:
        assert np.array_equal(np.asarray(g[k]), np.asarray(gt[k])), k
    assert not np.array_equal(c["g2"], c["g2"].T)


# ---------------------------------------------------------------------------------------------------------------- the collapsed bound
def _collapsed_case(N=40, M=6, D=2, DY=2, noisy=True, seed=5):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((N, D))
    s = rng.uniform(0.05, 0.3, (N, D)) if noisy else None
    Z = CR.spaced_points(rng, M, D, 0.5)
    Y = np.sin(mu @ rng.standard_normal((D, DY))) + 0.2 * rng.standard_normal((N, DY))
    return dict(mu=mu, s=s, Z=Z, variance=1.3, ls=np.array([0.9, 1.2]), Y=Y, noise=0.2)


def test_bound_adjoints_match_central_differences():
    c = _collapsed_case()
    bound, g, mag = R.collapsed_grad(c["mu"], c["s"], c["Z"], c["variance"], c["ls"], True, c["Y"], c["noise"], CR.JITTER, dtype=LD)
    x = lambda a: np.asarray(a, dtype=LD)
    F = lambda mu=x(c["mu"]), s=x(c["s"]), Z=x(c["Z"]), v=LD(c["variance"]), ls=x(c["ls"]), s2=LD(c["noise"]): \
        CR.collapsed(mu, s, Z, v, ls, c["Y"], s2, CR.JITTER, dtype=LD)["bound"]
    assert F() == bound
    # the chain's unit: the bound's adjoints pass through Sigma^-1 and Kuu^-1, so a difference is held to 1e-6 of mag
    _close(g["X_mean"], _central(lambda a: F(mu=a), c["mu"]), mag["X_mean"], rel=1e-6)
    _close(g["X_var"], _central(lambda a: F(s=a), c["s"]), mag["X_var"], rel=1e-6)
    _close(g["Z"], _central(lambda a: F(Z=a), c["Z"]), mag["Z"], rel=1e-6)
    _close(g["lengthscales"], _central(lambda a: F(ls=a), c["ls"]), mag["lengthscales"], rel=1e-6)
    _close(g["variance"], _central(lambda a: F(v=a[0]), np.array([c["variance"]])), mag["variance"], rel=1e-6)
    _close(g["lik_variance"], _central(lambda a: F(s2=a[0]), np.array([c["noise"]])), mag["lik_variance"], rel=1e-6)


def test_exact_gp_gradient_matches_central_differences_and_the_collapsed_bound_at_Z_equal_X():
    c = _collapsed_case(N=12, M=12, noisy=False, seed=6)
    ls = np.array([1.1])
    lml, g = R.exact_gp_grad(c["mu"], c["Y"], c["variance"], ls, c["noise"], dtype=LD)
    F = lambda v=LD(c["variance"]), l=LD(ls[0]), s2=LD(c["noise"]): R.exact_gp_grad(c["mu"], c["Y"], v, np.array([l], dtype=LD), s2, dtype=LD)[0]
    for key, fd in (("variance", (F(v=LD(c["variance"]) + H) - F(v=LD(c["variance"]) - H)) / (2 * H)),
                    ("lengthscales", (F(l=LD(ls[0]) + H) - F(l=LD(ls[0]) - H)) / (2 * H)),
                    ("lik_variance", (F(s2=LD(c["noise"]) + H) - F(s2=LD(c["noise"]) - H)) / (2 * H))):
        assert abs(float(g[key] - fd)) <= 1e-7 * (1.0 + abs(float(fd))), key
    # Z = X, zero input variance, no jitter: the collapsed bound is the exact marginal likelihood, and so are its gradients
    bound, gc, _ = R.collapsed_grad(c["mu"], None, c["mu"], c["variance"], ls, False, c["Y"], c["noise"], 0.0, dtype=LD)
    assert abs(float(bound - lml)) <= 1e-12 * abs(float(lml))
    for key in ("variance", "lengthscales", "lik_variance"):
        assert abs(float(np.sum(gc[key]) - g[key])) <= 1e-9 * (1.0 + abs(float(g[key]))), key


# ---------------------------------------------------------------------------------------------------------------- the public surface
def test_the_entry_point_is_declared_listed_and_built():
    from doubly_stochastic_dgp import _lib
    with open(os.path.join(ROOT, "include", "dsdgp.h")) as f:
        header = f.read()
    assert "int dsdgp_rbf_expectations_grad(dsdgp_ctx* ctx, const dsdgp_kernel* kern" in header
    assert "dsdgp_rbf_expectations_grad" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "dsdgp_rbf_expectations_grad")


def test_scipy_optimizer_refuses_a_model_that_is_not_collapsed():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.training import ScipyOptimizer
    rng = np.random.RandomState(3)
    X, Y = rng.randn(20, 1), rng.randn(20, 1)
    model = DGP(X, Y, X[:6].copy(), [RBF(1), RBF(1)], Gaussian(variance=0.1))
    with pytest.raises(NotImplementedError, match="DGP_Collapsed"):
        ScipyOptimizer().minimize(model, maxiter=1)


def test_scipy_optimizer_host_side_on_a_stand_in_objective():
    """the optimiser's own work — packing, the softplus chain rule, assignment through Parameter.assign, a failed factorisation as a
    step back, an untrainable parameter left alone — on a collapsed model whose gradients are a stand-in computed on the host:
    F = -sum (theta - target)^2 over the four parameters, and the second evaluation raises CholeskyError"""
    from doubly_stochastic_dgp._lib import CholeskyError
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    from doubly_stochastic_dgp.training import ScipyOptimizer

    class StandIn(DGP_Collapsed):
        def compute_log_likelihood_gradients(self, zs=None):
            object.__setattr__(self, "_calls", getattr(self, "_calls", 0) + 1)
            if self._calls == 2:
                raise CholeskyError("stand-in: not positive definite")
            top, lik = self.layers[-1], self.likelihood.likelihood
            params = [top.feature.Z, top.kern.variance, top.kern.lengthscales, lik.variance]
            targets = [np.full(top.feature.Z.shape, 0.25), 2.0, 0.7, 0.3]
            bound = -sum(float(np.sum((p.value - t) ** 2)) for p, t in zip(params, targets))
            return bound, [(p, -2.0 * (p.value - t)) for p, t in zip(params, targets)], {}

    rng = np.random.RandomState(4)
    X, Y = rng.randn(20, 2), rng.randn(20, 1)
    kern, lik = RBF(2, lengthscales=2.0), Gaussian(variance=1.0)
    top = SGPR_Layer(kern, X[:5].copy(), 1, Zero())
    model = StandIn(X, Y, lik, [top])
    kern.lengthscales.set_trainable(False)
    res = ScipyOptimizer(tol=1e-12).minimize(model, maxiter=200)
    assert res.success and model._calls > 2 and res.x.size == 5 * 2 + 2 and np.isfinite(res.fun)
    assert np.allclose(top.feature.Z.value, 0.25, atol=1e-5) and abs(float(kern.variance.value) - 2.0) < 1e-5
    assert abs(float(lik.variance.value) - 0.3) < 1e-5
    assert float(np.asarray(kern.lengthscales.value).reshape(-1)[0]) == 2.0           # not trainable: its bits stay
    # a failure at the starting point has nothing to step back to: it is raised
    object.__setattr__(model, "_calls", 1)
    with pytest.raises(CholeskyError):
        ScipyOptimizer().minimize(model, maxiter=5)
    for p in (top.feature.Z, kern.variance, lik.variance):
        p.set_trainable(False)
    with pytest.raises(ValueError, match="trainable"):
        ScipyOptimizer().minimize(model)


def test_collapsed_model_keeps_refusing_the_engine_optimisers():
    """the new capability arrives through new names only: supports_gradients stays False"""
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    assert DGP_Collapsed.supports_gradients is False and callable(DGP_Collapsed.compute_log_likelihood_gradients)
