"""-m gpu: layers.SGPMC_Layer and a DGP_Collapsed over it.

  * the layer's conditional_ND and conditional_vjp against tests/sparse_cond_reference.py with the project's bar, 8 max(e64, 2^-50 mag)
    (jitter variance M / 50, as tests/sparse_cond_cases.py), Zero / Identity / fixed Linear mean;
  * Z = X, white=True, a GPR_Layer on top: the model is DGP_Heinonen's up to the jitter (A = Lu^-1 (Lu Lu^T - jitter I) = Lu^T - jitter
    Lu^-1, and the top layer does not read the variance).  The bar is the distance of the two routes in float64 on the CPU
    (tests/dense_reference.py's log density against the sparse conditional under the same GPR bound): the device's two models differ by
    that same jitter term plus rounding that is orders smaller, so twice the CPU's distance holds it and excludes a term of any other
    order;
  * an SGPR_Layer on top: every gradient pair against central differences of the device's own log density, with the step and the bar of
    tests/test_gpu_collapsed_train.py: h = 1e-4, 4 |fd(h) - fd(h / 2)| + 1e-9 |log density| / h;
  * ScipyOptimizer(inner=True) raises the log density; predictions have their shapes and are finite;
  * HMC: the leapfrog is reversible and of second order, as tests/test_gpu_hmc.py holds the dense model; a run replayed from its seed
    gives the same bits."""
import numpy as np
import pytest

from tests import dense_reference as DR
from tests import gram_grad_reference as GR
from tests import sparse_cond_reference as SR

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _ratio(dev, tr, f64, mag):
    dev, tr, f64, mag = (np.atleast_1d(np.asarray(a)) for a in (dev, tr, f64, mag))
    err = np.abs(dev - tr).astype(np.float64)
    bar = 8.0 * np.maximum(np.abs(f64 - tr).astype(np.float64), 2.0 ** -50 * mag.astype(np.float64))
    if np.any((bar == 0.0) & (err != 0.0)) or np.any(np.isnan(err)):
        return float("inf")
    return float(np.max(err / np.where(bar == 0.0, 1.0, bar)))


#            kind         ard white_var white  n   M   D  DO mean
LAYER_CASES = {
    "zero":     (GR.RBF,      1, None, True,  70, 17, 3, 2, None),
    "identity": (GR.MATERN52, 0, 0.2,  False, 65, 12, 2, 2, "identity"),
    "linear":   (GR.RBF,      0, None, False, 33, 9,  2, 3, "linear"),
}


@pytest.mark.parametrize("name", list(LAYER_CASES))
def test_layer_conditional_and_vjp_match_the_reference(name):
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.gpflow_compat import RBF, Identity, Linear, Matern52, White, Zero
    from doubly_stochastic_dgp.layers import SGPMC_Layer
    kind, ard, wv, white, n, M, D, DO, mean = LAYER_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    Z, X, q = rng.standard_normal((M, D)), rng.standard_normal((n, D)), rng.standard_normal((M, DO))
    ls, variance = np.sqrt(D) * rng.uniform(0.7, 1.4, D if ard else 1), 1.3
    gm, gv2 = rng.standard_normal((n, DO)), rng.standard_normal((n, DO))
    jitter = variance * M / 50.0
    A = rng.standard_normal((D, DO))
    b = rng.standard_normal(DO)
    kern = (RBF if kind == GR.RBF else Matern52)(D, variance=variance, lengthscales=ls if ard else float(ls[0]), ARD=bool(ard))
    if wv is not None:
        kern = kern + White(D, variance=wv)
    mf = Zero() if mean is None else Identity() if mean == "identity" else Linear(A=A, b=b)
    mf.set_trainable(False)
    layer = SGPMC_Layer(kern, Z, DO, mf, white=white)
    layer.q_mu = q
    ref_mean = None if mean is None else "identity" if mean == "identity" else (A, b)
    with settings.temp_jitter(jitter):
        m, v = layer.conditional_ND(X)
        m_full, cov = layer.conditional_ND(X, full_cov=True)
        g = layer.conditional_vjp(gm, gv2.sum(1))                   # dvar already summed over the outputs; X: the last conditional's
        g_x = layer.conditional_vjp(gm, gv2.sum(1), X=X)
        g_2d = layer.conditional_vjp(gm, gv2, X=X)                  # dvar per output: summed on the device, in another order
    assert v.shape == (n, DO) and all(np.array_equal(v[:, 0], v[:, d]) for d in range(DO))
    assert cov.shape == (n, n, DO) and np.array_equal(cov[:, :, 0], cov[:, :, DO - 1])
    for k in g:
        assert np.array_equal(_bits(g[k]), _bits(g_x[k])), k
        assert np.max(np.abs(np.asarray(g_2d[k]) - np.asarray(g[k]))) <= 1e-12 * (1.0 + np.max(np.abs(g[k]))), k
    assert ("white_variance" in g) == (wv is not None)
    figs = {}
    ref = {}
    for dt in (LD, np.float64):
        (f, fmag), (r, rmag) = SR.forward(kind, Z, X, q, variance, ls, wv, jitter, white, dtype=dt), \
            SR.reverse(kind, Z, X, q, variance, ls, bool(ard), wv, jitter, white, gm, gv2.sum(1), dtype=dt)
        c, cmag = SR.full_cov(kind, Z, X, q, variance, ls, wv, jitter, white, dtype=dt)
        ms = DR.mean_fn(ref_mean, X, dt)
        mu, mum = (f["mean"], fmag["mean"]) if ms is None else (f["mean"] + ms, fmag["mean"] + np.abs(ms))
        dX, dXm = r["X"], rmag["X"]
        if mean == "identity":
            dX, dXm = dX + np.asarray(gm, dtype=dt), dXm + np.abs(gm)
        elif mean == "linear":
            dX, dXm = dX + np.asarray(gm, dtype=dt) @ np.asarray(A, dtype=dt).T, dXm + np.abs(gm) @ np.abs(A).T
        ref[dt] = (dict(mean=mu, var=f["var"], cov=c, q_mu=r["q_mu"], Z=r["Z"], X=dX, variance=r["variance"], lengthscales=r["lengthscales"],
                        white_variance=r["diag"]),
                   dict(mean=mum, var=fmag["var"], cov=cmag, q_mu=rmag["q_mu"], Z=rmag["Z"], X=dXm, variance=rmag["variance"],
                        lengthscales=rmag["lengthscales"], white_variance=rmag["diag"]))
    (tr, mag), (f64, _) = ref[LD], ref[np.float64]
    got = dict(g, mean=m, var=v[:, 0], cov=cov[:, :, 0], mean_full=m_full)      # full_cov: the mean by dsdgp_gemm, another summation order
    for d in (tr, f64, mag):
        d["mean_full"] = d["mean"]
    for k in got:
        figs[k] = _ratio(got[k], tr[k], f64[k], mag[k])
    print(name + ": " + ", ".join("%s %.3g" % kv for kv in figs.items()) + " (x bar)")
    for k, fig in figs.items():
        assert fig <= 1.0, (k, fig)


N, DX, DY = 24, 2, 1


def _data(seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, (N, DX))
    Y = np.sin(2.0 * X[:, :1]) + 0.3 * X[:, 1:] + 0.1 * rng.standard_normal((N, DY))
    return rng, X, Y


def _sparse_model(seed=3, M=7, top="sgpr", q_scale=0.5, lik_var=0.1):
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Identity, White, Zero
    from doubly_stochastic_dgp.layers import GPR_Layer, SGPMC_Layer, SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    rng, X, Y = _data(seed)
    low = SGPMC_Layer(RBF(DX, variance=0.8, lengthscales=np.array([1.1, 0.9]), ARD=True) + White(DX, variance=0.05), X[:M].copy(), DX,
                      Identity(), white=True)
    low.q_mu = q_scale * rng.standard_normal((M, DX))
    if top == "sgpr":
        upper = SGPR_Layer(RBF(DX, variance=1.2, lengthscales=1.3), X[M:2 * M].copy() + 0.1, DY, Zero())
    else:
        upper = GPR_Layer(RBF(DX, variance=1.2, lengthscales=1.3), Zero(), DY)
    return DGP_Collapsed(X, Y, Gaussian(variance=lik_var), [low, upper]), rng, X, Y


def test_with_z_at_x_the_model_is_heinonens_up_to_the_jitter():
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, Matern52, RBF, Zero
    from doubly_stochastic_dgp.layers import GPMC_Layer, GPR_Layer, SGPMC_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed, DGP_Heinonen
    rng, X, Y = _data(11)
    q = rng.standard_normal((N, DX))
    ls0, ls1, s2, jitter = np.array([0.8]), np.array([1.2]), 0.05, settings.jitter
    kern0 = lambda: Matern52(DX, variance=0.9, lengthscales=float(ls0[0]))
    kern1 = lambda: RBF(DX, variance=1.1, lengthscales=float(ls1[0]))
    dense = DGP_Heinonen(X, Y, Gaussian(variance=s2), [GPMC_Layer(kern0(), X.copy(), DX, Zero()), GPR_Layer(kern1(), Zero(), DY)])
    sparse = DGP_Collapsed(X, Y, Gaussian(variance=s2), [SGPMC_Layer(kern0(), X.copy(), DX, Zero(), white=True), GPR_Layer(kern1(), Zero(), DY)])
    dense.layers[0].q_mu = q
    sparse.layers[0].q_mu = q
    # the two routes in float64 on the CPU
    v_dense, g_dense, _ = DR.log_density((GR.MATERN52, GR.RBF), X, Y, q, 0.9, ls0, jitter, 1.1, ls1, False, s2, dtype=np.float64)
    f, _ = SR.forward(GR.MATERN52, X, X, q, 0.9, ls0, None, jitter, True, dtype=np.float64)
    r, _ = DR.gpr(GR.RBF, f["mean"], Y, 1.1, ls1, False, None, s2, dtype=np.float64)
    rev, _ = SR.reverse(GR.MATERN52, X, X, q, 0.9, ls0, False, None, jitter, True, r["X_mean"], np.zeros(N), dtype=np.float64)
    v_sparse = r["bound"][0] - 0.5 * np.sum(q * q) - 0.5 * q.size * np.log(2.0 * np.pi)
    g_sparse = rev["q_mu"] - q
    bar_v, bar_g = 2.0 * abs(v_sparse - v_dense), 2.0 * np.max(np.abs(g_sparse - g_dense))
    d_v, d_pairs = dense.compute_log_density_gradients()
    s_v, s_pairs = sparse.compute_log_density_gradients()
    assert sparse.compute_log_density() == s_v
    g_d = next(g for p, g in d_pairs if p is dense.layers[0].q_mu)
    g_s = next(g for p, g in s_pairs if p is sparse.layers[0].q_mu)
    print("log density: dense %.15g, sparse %.15g, |difference| %.3g (bar %.3g); q_mu gradient: max |difference| %.3g (bar %.3g)"
          % (d_v, s_v, abs(d_v - s_v), bar_v, np.max(np.abs(g_d - g_s)), bar_g))
    assert bar_v > 0.0 and bar_g > 0.0
    assert abs(d_v - s_v) <= bar_v
    assert np.max(np.abs(g_d - g_s)) <= bar_g


def test_pairs_names_and_order():
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    model, rng, X, Y = _sparse_model()
    low, top = model.layers
    stat, wk = split_kernel(low.kern)
    bound, pairs, adj = model.compute_log_likelihood_gradients(inner=True)
    want = [top.feature.Z, top.kern.variance, top.kern.lengthscales, model.likelihood.likelihood.variance,
            low.feature.Z, low.q_mu, stat.variance, stat.lengthscales, wk.variance]
    assert len(pairs) == len(want) and all(p is w and g.shape == p.shape for (p, g), w in zip(pairs, want))
    assert bound == model.compute_log_likelihood() and adj["X_mean"].shape == (N, DX) and adj["X_var"].shape == (N, DX)
    b4, p4, _ = model.compute_log_likelihood_gradients()
    assert b4 == bound and len(p4) == 4 and all(np.array_equal(_bits(g), _bits(h)) for (_, g), (_, h) in zip(p4, pairs))
    value, dpairs = model.compute_log_density_gradients()
    assert value == bound + model.compute_log_prior() == model.compute_log_density()
    assert np.array_equal(_bits(dpairs[5][1]), _bits(pairs[5][1] - low.q_mu.value))
    with pytest.raises(RuntimeError):
        model.inner_engine()


def test_every_gradient_pair_against_central_differences_of_the_devices_own_log_density():
    model, rng, X, Y = _sparse_model()
    value, pairs = model.compute_log_density_gradients()
    h = 1e-4

    def fd(p, idx, step):
        base = p.value.copy()
        vals = []
        for sign in (1.0, -1.0):
            v = base.copy()
            v[idx] += sign * step
            p.assign(v)
            vals.append(model.compute_log_density())
        p.assign(base)
        return (vals[0] - vals[1]) / (2.0 * step)

    for n_pair, (p, g) in enumerate(pairs):
        entries = list(np.ndindex(p.shape))
        for idx in [entries[i] for i in rng.choice(len(entries), size=min(3, len(entries)), replace=False)]:
            f1, f2 = fd(p, idx, h), fd(p, idx, h / 2)
            bar = 4.0 * abs(f1 - f2) + 1e-9 * abs(value) / h
            print("pair %d %s: gradient %.10g, central difference %.10g, bar %.3g" % (n_pair, idx, g[idx], f2, bar))
            assert abs(g[idx] - f2) <= bar, (n_pair, idx)


@pytest.mark.parametrize("top", ("sgpr", "gpr"))
def test_lbfgs_raises_the_log_density_and_the_model_predicts(top):
    from doubly_stochastic_dgp.training import ScipyOptimizer
    model, rng, X, Y = _sparse_model(top=top)
    before = model.compute_log_density()
    res = ScipyOptimizer().minimize(model, maxiter=8, inner=True)
    after = model.compute_log_density()
    print("%s: log density %.6f -> %.6f in %d iterations" % (top, before, after, res.nit))
    assert after > before and abs(after + res.fun) <= 1e-9 * abs(after)
    Xs = rng.uniform(-1.5, 1.5, (5, DX))
    m, v = model.predict_y(Xs, 2)
    fm, fv = model.predict_f(Xs, 2)
    ffm, ffv = model.predict_f_full_cov(Xs, 1)
    dens = model.predict_density(Xs, np.zeros((5, DY)), 2)
    Fs, Fm, Fv = model.predict_all_layers(Xs, 2)
    assert m.shape == v.shape == fm.shape == fv.shape == (2, 5, DY) and ffv.shape == (1, 5, 5, DY) and dens.shape == (5, DY)
    assert [f.shape for f in Fs] == [(2, 5, DX), (2, 5, DY)] and len(Fm) == len(Fv) == 2
    assert all(np.all(np.isfinite(a)) for a in (m, v, fm, fv, ffm, ffv, dens)) and np.all(v > 0.0)


def test_hmc_leapfrog_is_reversible_and_second_order_and_a_run_replays_from_its_seed():
    from doubly_stochastic_dgp.training import HMC
    model, rng, X, Y = _sparse_model(lik_var=4.0)      # a wide likelihood: eps = 0.1 is inside the integrator's asymptotic range
    q0 = model.layers[0].q_mu.value.copy()
    p0 = np.random.default_rng(9).standard_normal(q0.shape)
    q1, p1, _ = HMC.leapfrog(model, q0, p0, 0.05, 8)
    q2, p2, _ = HMC.leapfrog(model, q1, -p1, 0.05, 8)
    print("return error: q %.3g, p %.3g" % (np.max(np.abs(q2 - q0)), np.max(np.abs(-p2 - p0))))
    assert np.max(np.abs(q2 - q0)) <= 1e-12 and np.max(np.abs(-p2 - p0)) <= 1e-12
    assert np.max(np.abs(q1 - q0)) > 1e-2
    model.layers[0].q_mu = q0
    H0 = -model.compute_log_density() + 0.5 * np.sum(p0 ** 2)
    err = {}
    for eps, steps in ((0.1, 4), (0.05, 8), (0.025, 16), (0.0125, 32)):
        q, p, logp = HMC.leapfrog(model, q0, p0, eps, steps)
        err[eps] = abs((-logp + 0.5 * np.sum(p * p)) - H0)
    for eps in (0.1, 0.05, 0.025):
        ratio = err[eps] / err[eps / 2]
        print("energy error ratio at eps = %g: %.4f" % (eps, ratio))
        assert 3.5 <= ratio <= 4.5, (eps, ratio)
    model.layers[0].q_mu = q0
    out = HMC().sample(model, 4, 0.05, lmin=1, lmax=3, seed=5)
    assert out["samples"]["q_mu"].shape == (4,) + q0.shape and np.array_equal(model.layers[0].q_mu.value, out["samples"]["q_mu"][-1])
    model.layers[0].q_mu = q0
    again = HMC().sample(model, 4, 0.05, lmin=1, lmax=3, seed=5)
    assert np.array_equal(_bits(again["samples"]["q_mu"]), _bits(out["samples"]["q_mu"]))
    assert again["accepted"].tolist() == out["accepted"].tolist() and np.array_equal(_bits(again["logprobs"]), _bits(out["logprobs"]))
