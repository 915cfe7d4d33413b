"""-m gpu: the dense layers on the device (layers.GPR_Layer, layers.GPMC_Layer; dsdgp_gpr_bound, dsdgp_gpr_var and the primitives they
compose) against tests/dense_reference.py.

Bars, by the project's rule: the truth is long double; e64 is the distance of the same operation sequence in float64 numpy from it, entry
by entry; mag is the sum of the magnitudes of the terms added into the entry; the device is within 8 max(e64, 2^-50 mag).  The noise
variance is 1e-2 or more, so that the reference's own conditioning stays inside the bar.  GPMC_Layer hands out its factor Lu itself
(latents = Lu q_mu, vjp = Lu^T dF), and the forward error of a Cholesky factor is cond(K) u, whichever route computes it; the bar resolves
2^-50 = 8 u, 64 u with its factor 8.  So its cases get a jitter of variance N / 50 (settings.temp_jitter): cond(k(X, X) + jitter I) <=
(variance N + jitter) / jitter = 51, and what the factor loses stays below what the bar resolves.  (The factorisation on ill-conditioned
matrices has its own tests: tests/test_gpu_factor_direct.py.)  Cases: N in {6, 17, 130} (130: two row blocks
of the reverse pass of the Gram matrix, three column splits), DY in {1, 2}, Zero / Identity / Linear mean, both kernels, with and without
a White part, scalar and ARD lengthscales.  The gradient is also held, at one entry of each block, against central differences of the
device's own bound."""
import numpy as np
import pytest

from tests import dense_reference as DR
from tests import gram_grad_reference as GR

pytestmark = pytest.mark.gpu
LD = np.longdouble

#          N   D  DY kind         ard white  mean        s2   seed
CASES = {
    "n6":   (6,  3, 2, GR.MATERN52, 0, None, None,       0.01, 1),
    "n17":  (17, 2, 2, GR.RBF,      1, None, "identity", 0.05, 2),
    "n17w": (17, 3, 1, GR.RBF,      0, 0.3,  None,       0.01, 3),
    "n130": (130, 3, 1, GR.MATERN52, 1, 0.2, "linear",   0.1,  4),
    "n130z": (130, 3, 2, GR.RBF,    1, None, None,       0.02, 5),
}
NS = 7


def _inputs(name):
    N, D, DY, kind, ard, white, mean, s2, seed = CASES[name]
    rng = np.random.default_rng(100 + seed)
    F, Y, Xs = rng.standard_normal((N, D)), rng.standard_normal((N, DY)), rng.standard_normal((NS, D))
    ls = np.sqrt(D) * rng.uniform(0.5, 1.5, D if ard else 1)
    if mean == "linear":
        mean = (rng.standard_normal((D, DY)), rng.standard_normal(DY))
    return dict(N=N, D=D, DY=DY, kind=kind, ard=bool(ard), white=white, mean=mean, s2=s2, F=F, Y=Y, Xs=Xs, ls=ls, variance=1.3, rng=rng)


def _kernel(c):
    from doubly_stochastic_dgp.gpflow_compat import RBF, Matern52, White
    k = (RBF if c["kind"] == GR.RBF else Matern52)(c["D"], variance=c["variance"], lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]),
                                                  ARD=c["ard"])
    return k if c["white"] is None else k + White(c["D"], variance=c["white"])


def _mean(c):
    from doubly_stochastic_dgp.gpflow_compat import Identity, Linear, Zero
    if c["mean"] is None:
        return Zero()
    if isinstance(c["mean"], str):
        return Identity()
    mf = Linear(A=c["mean"][0], b=c["mean"][1])
    mf.set_trainable(False)
    return mf


def _ratio(dev, tr, f64, mag):
    dev, tr, f64, mag = (np.atleast_1d(np.asarray(a)) for a in (dev, tr, f64, mag))
    err = np.abs(dev - tr).astype(np.float64)
    bar = 8.0 * np.maximum(np.abs(f64 - tr).astype(np.float64), 2.0 ** -50 * mag.astype(np.float64))
    if np.any((bar == 0.0) & (err != 0.0)) or np.any(np.isnan(err)):
        return float("inf")
    return float(np.max(err / np.where(bar == 0.0, 1.0, bar)))


def _hold(name, got, tr, f64, mag, keys):
    figs = {k: _ratio(got[k], tr[k], f64[k], mag[k]) for k in keys}
    print(name + ": " + ", ".join("%s %.3g" % kv for kv in figs.items()) + " (x bar)")
    for k, fig in figs.items():
        assert fig <= 1.0, (name, k, fig)


@pytest.mark.parametrize("name", list(CASES))
def test_gpr_layer_matches_the_reference(name):
    from doubly_stochastic_dgp.layers import GPR_Layer
    c = _inputs(name)
    ref = lambda dt: DR.gpr(c["kind"], c["F"], c["Y"], c["variance"], c["ls"], c["ard"], c["white"], c["s2"], c["mean"], Xnew=c["Xs"], dtype=dt)
    (tr, mag), (f64, _) = ref(LD), ref(np.float64)
    layer = GPR_Layer(_kernel(c), _mean(c), c["DY"])
    layer.set_data(c["F"], None, c["Y"], c["s2"])
    bound, terms = layer.bound_terms()
    g = layer.bound_gradients()
    assert g["bound"] == bound == layer.build_likelihood() and np.all(g["X_var"] == 0.0) and g["X_var"].shape == c["F"].shape
    assert ("white_variance" in g) == (c["white"] is not None)
    got = dict(g, terms=terms, bound=bound)
    keys = ["bound", "terms", "variance", "lengthscales", "lik_variance", "X_mean"] + (["white_variance"] if c["white"] is not None else [])
    mean, var = layer.conditional_ND(c["Xs"])
    mean_f, cov = layer.conditional_ND(c["Xs"], full_cov=True)
    assert var.shape == (NS, c["DY"]) and cov.shape == (NS, NS, c["DY"]) and np.array_equal(mean, mean_f)
    assert all(np.array_equal(cov[:, :, 0], cov[:, :, d]) for d in range(c["DY"]))
    got.update(mean=mean, var=var, cov=cov[:, :, 0])
    _hold(name, got, tr, f64, mag, keys + ["mean", "var", "cov"])
    # the same data give the same bits
    again = layer.bound_gradients()
    assert all(np.array_equal(np.atleast_1d(again[k]), np.atleast_1d(g[k])) for k in g)


@pytest.mark.parametrize("name", ("n17", "n130"))
def test_gpr_gradient_matches_central_differences_of_the_device_bound(name):
    """one entry of each block.  The device's bound carries a rounding error of a few 2^-50 of its terms' magnitudes (some 1e-13 here);
    over 2 h = 2e-5 that is 1e-8, and the truncation h^2 / 6 |F'''| is smaller: 1e-6 (1 + |g|) holds both with room and still excludes a
    wrong factor or sign"""
    from doubly_stochastic_dgp.layers import GPR_Layer
    c = _inputs(name)
    h = 1e-5

    def bound(F=None, variance=None, ls=None, s2=None, white=None):
        cc = dict(c, variance=variance or c["variance"], ls=c["ls"] if ls is None else ls, white=white or c["white"])
        layer = GPR_Layer(_kernel(cc), _mean(cc), c["DY"])
        layer.set_data(c["F"] if F is None else F, None, c["Y"], s2 or c["s2"])
        return layer, layer.build_likelihood()

    layer, _ = bound()
    g = layer.bound_gradients()

    def fd(**kw):
        (k, (lo, hi)), = kw.items()
        return (bound(**{k: hi})[1] - bound(**{k: lo})[1]) / (2 * h)

    def bump(a, idx, s):
        b = np.array(a, dtype=np.float64)
        b[idx] += s * h
        return b

    checks = [("X_mean", g["X_mean"][3, 1], fd(F=(bump(c["F"], (3, 1), -1), bump(c["F"], (3, 1), 1)))),
              ("variance", g["variance"], fd(variance=(c["variance"] - h, c["variance"] + h))),
              ("lengthscales", np.atleast_1d(g["lengthscales"])[0], fd(ls=(bump(c["ls"], 0, -1), bump(c["ls"], 0, 1)))),
              ("lik_variance", g["lik_variance"], fd(s2=(c["s2"] - h, c["s2"] + h)))]
    if c["white"] is not None:
        checks.append(("white_variance", g["white_variance"], fd(white=(c["white"] - h, c["white"] + h))))
    for k, want, got in checks:
        print("%s %s: gradient %.10g, central difference %.10g" % (name, k, want, got))
        assert abs(got - want) <= 1e-6 * (1.0 + abs(want)), k


def test_gpr_layer_refuses_a_trainable_linear_mean_and_a_matrix_that_is_not_positive_definite():
    from doubly_stochastic_dgp._lib import CholeskyError
    from doubly_stochastic_dgp.gpflow_compat import Linear
    from doubly_stochastic_dgp.layers import GPR_Layer
    c = _inputs("n17")
    layer = GPR_Layer(_kernel(c), Linear(A=np.ones((c["D"], c["DY"]))), c["DY"])
    layer.set_data(c["F"], None, c["Y"], c["s2"])
    assert np.isfinite(layer.build_likelihood())
    with pytest.raises(NotImplementedError):
        layer.bound_gradients()
    with pytest.raises(CholeskyError):
        layer.set_data(c["F"], None, c["Y"], -10.0)                 # k(F, F) - 10 I
    with pytest.raises(RuntimeError):                              # the layer holds no data
        layer.build_likelihood()
    with pytest.raises(RuntimeError):
        layer.conditional_ND(c["Xs"])


@pytest.mark.parametrize("name,prop", (("n6", None), ("n17", None), ("n130", 2)))
def test_gpmc_layer_matches_the_reference(name, prop):
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.layers import GPMC_Layer
    c = _inputs(name)
    N, D, DO = c["N"], c["D"], c["DY"]
    q_mu, dF = c["rng"].standard_normal((N, DO)), c["rng"].standard_normal((N, DO))
    jitter = c["variance"] * N / 50.0                       # cond <= 51: see the module's docstring
    ref = lambda dt: DR.gpmc(c["kind"], c["F"], q_mu, c["variance"], c["ls"], c["white"], jitter, c["mean"], dF=dF, Xnew=c["Xs"], dtype=dt)
    (tr, mag), (f64, _) = ref(LD), ref(np.float64)
    with settings.temp_jitter(jitter):
        layer = GPMC_Layer(_kernel(c), c["F"], DO, _mean(c), input_prop_dim=prop)
    assert layer.q_mu.shape == (N, DO) and np.all(layer.q_mu.value == 0.0) and layer.KL() == 0.0
    assert layer.log_prior() == -0.5 * N * DO * np.log(2.0 * np.pi)
    layer.q_mu = q_mu
    assert abs(layer.log_prior() - (-0.5 * np.sum(q_mu ** 2) - 0.5 * N * DO * np.log(2.0 * np.pi))) <= 1e-12 * N * DO
    p = prop or 0
    f = layer.build_latents()
    assert f.shape == (N, p + DO) and np.array_equal(f[:, :p], c["F"][:, :p])
    vjp = layer.latents_vjp(np.concatenate([np.full((N, p), 1e300), dF], 1))      # the propagated columns' adjoints are dropped
    mean, var = layer.conditional_ND(c["Xs"])
    mean_f, cov = layer.conditional_ND(c["Xs"], full_cov=True)
    assert var.shape == (NS, DO) and cov.shape == (NS, NS, DO) and np.array_equal(mean, mean_f)
    got = dict(latents=f[:, p:], vjp=vjp, mean=mean, var=var, cov=cov[:, :, 0])
    _hold(name, got, tr, f64, mag, ["latents", "vjp", "mean", "var", "cov"])
