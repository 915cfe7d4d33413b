"""-m gpu: DGP_Base.sample_functions (doubly_stochastic_dgp/pathwise.py) at the model level against tests/pathwise_reference.py, the
draw's normals replayed on the CPU through oracle/philox.py in the documented streams and layouts.

Layer by layer: each layer's reference is fed the device's own previous-layer output, and every entry is within the project's bar
8 max(e64, 2^-50 mag) of the long-double truth (tests/test_gpu_pathwise.py).  End to end: the largest distance of the device's last layer
from the truth composed in long double is within 8 times the largest distance of the float64 twin composed the same way.  Bits: any
batch size and any split of the inputs into calls give the same bits; a training step after the draw changes nothing.  Moments: on the
configuration of tests/pathwise_cases.py the sample mean and covariance over 4096 draws are within 5 standard errors of the exact
moments given the basis (tests/test_pathwise_reference_cpu.py holds the float64 twin to 4)."""
import numpy as np
import pytest

from tests import pathwise_cases as PC
from tests import pathwise_reference as PR

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _model(depth, white, seed=0):
    """two layers: D = 3 -> 3 (Identity) -> 1 (Zero), M = 16; three layers: D = 4 -> 2 (Linear, PCA) -> 2 (Identity) -> 1, M = 24"""
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Matern52, White
    rng = np.random.default_rng(seed)
    if depth == 2:
        D, M, kernels = 3, 16, [RBF(3, variance=1.2, lengthscales=[0.9, 1.2, 1.5], ARD=True), Matern52(3, lengthscales=1.3) + White(3, 0.05)]
    else:
        D, M = 4, 24
        kernels = [Matern52(4, variance=0.8, lengthscales=[1.5, 1.0, 2.0, 1.2], ARD=True), RBF(2, lengthscales=0.9) + White(2, 0.1),
                   RBF(2, variance=1.5, lengthscales=1.1) + White(2, 0.05)]
    X = 1.5 * rng.standard_normal((48, D))
    Y = rng.standard_normal((48, 1))
    model = DGP(X, Y, X[:M].copy(), kernels, Gaussian(), white=white, num_samples=2)
    for layer in model.layers:
        Ml, DO = layer.q_mu.shape
        layer.q_mu = rng.standard_normal((Ml, DO))
        layer.q_sqrt = np.tril(0.2 * rng.standard_normal((DO, Ml, Ml))) + 0.5 * np.eye(Ml)[None]
    return model, X


def _layer_params(model):
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    out = []
    for layer in model.layers:
        stat, white = split_kernel(layer.kern)
        mf = layer.mean_function
        out.append(dict(kind=stat.kind, D=stat.input_dim, variance=float(stat.variance.value),
                        ls=np.array(stat.lengthscales.value, dtype=np.float64).reshape(-1),
                        white_var=None if white is None else float(white.variance.value), Z=np.array(layer.feature.Z.value),
                        q_mu=np.array(layer.q_mu.value), q_sqrt=np.array(layer.q_sqrt.value), white=layer.white, mean=mf.kind,
                        A=np.array(mf.A.value) if mf.kind == "linear" else None, b=np.array(mf.b.value) if mf.kind == "linear" else None,
                        jitter=float(settings.jitter)))
    return out


def _reference_layer(p, Om, normals, Xin, dtype):
    """((S, n, DO), mag) of one layer at Xin (n, D) or (S, n, D)"""
    Wc, Ws, eps = normals
    V, _ = PR.weights(p["kind"], p["Z"], Om, p["Z"][0], Wc, Ws, p["q_mu"], p["q_sqrt"], eps, p["variance"], p["ls"], p["white_var"],
                      p["jitter"], p["white"], dtype)
    Xin = np.asarray(Xin, dtype=dtype)
    add = None if p["mean"] == "zero" else Xin if p["mean"] == "identity" else Xin @ np.asarray(p["A"], dtype=dtype) + np.asarray(p["b"], dtype=dtype)
    return PR.evaluate(p["kind"], Xin, Om, p["Z"][0], Wc, Ws, p["Z"], V, p["variance"], p["ls"], add, dtype)


@pytest.mark.parametrize("depth,white,S,L", [(2, False, 3, 40), (3, True, 4, 33)])
def test_every_layer_matches_the_reference_and_the_stack_end_to_end(depth, white, S, L):
    model, X = _model(depth, white)
    seed = 7
    fs = model.sample_functions(num_functions=S, num_features=L, seed=seed)
    Xs = X[:37] + 0.1
    dev = fs.all_layers(Xs)
    params = _layer_params(model)
    rng = np.random.default_rng(seed)
    truth_in, twin_in = Xs, Xs
    for l, p in enumerate(params):
        Om = PR.sample_basis(p["kind"], p["D"], L, p["ls"], rng)
        assert _same_bits(Om, fs.layers[l].Omega_host)
        normals = PR.replay_normals(seed, l, S, L, p["Z"].shape[0], p["q_mu"].shape[1])
        fed = Xs if l == 0 else dev[l - 1]
        (tr, mag), (tw, _) = _reference_layer(p, Om, normals, fed, PR.LD), _reference_layer(p, Om, normals, fed, np.float64)
        assert dev[l].shape == tr.shape
        fig = PR.ratio(dev[l], tr, tw, mag)
        print(f"depth {depth}, layer {l} ({p['kind']}, {p['mean']}): {fig:.3g} (x bar)")
        assert fig <= 1.0, (l, fig)
        truth_in = _reference_layer(p, Om, normals, truth_in, PR.LD)[0]
        twin_in = _reference_layer(p, Om, normals, twin_in, np.float64)[0]
    d_dev = float(np.max(np.abs(dev[-1] - truth_in)))
    d_twin = float(np.max(np.abs(twin_in - truth_in)))
    print(f"depth {depth} end to end: device {d_dev:.3g}, twin {d_twin:.3g}")
    assert d_dev <= 8.0 * d_twin


def test_batches_and_splits_give_the_same_bits_and_training_changes_nothing():
    model, X = _model(3, False)
    fs = model.sample_functions(num_functions=3, num_features=48, seed=1)
    Xs = X[:40] - 0.2
    full = fs.all_layers(Xs)
    small = fs.all_layers(Xs, batch_size=7)
    for a, b in zip(full, small):
        assert _same_bits(a, b)
    Xa, Xb = Xs[:13], Xs[13:]
    assert _same_bits(fs(np.concatenate([Xa, Xb])), np.concatenate([fs(Xa), fs(Xb)], axis=1))
    on_dev = fs(Xs, on_device=True)
    model._context().sync()
    assert _same_bits(on_dev.cpu().numpy(), full[-1])
    assert _same_bits(fs(model._context().to_device(Xs)), full[-1])
    before = [np.array(layer.q_mu.value) for layer in model.layers]
    model.train_step(0.05, sync=True)
    assert any(not np.array_equal(b, np.array(layer.q_mu.value)) for b, layer in zip(before, model.layers))
    assert _same_bits(fs(Xs), full[-1])                      # a snapshot
    again = model.sample_functions(num_functions=3, num_features=48, seed=1)
    assert not _same_bits(again(Xs), full[-1])               # the trained model's draw is another one
    assert fs.basis_error(0) > 0.0 and fs.basis_error(0) == fs.basis_error(0)


def _moment_model():
    from doubly_stochastic_dgp.dgp import DGP_Base
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SVGP_Layer
    c = PC.moment_config()
    layer = SVGP_Layer(RBF(2, variance=c["variance"], lengthscales=float(c["ls"][0])), c["Z"], 1, Zero(), white=False)
    layer.q_mu, layer.q_sqrt = c["q_mu"], c["q_sqrt"]
    return DGP_Base(c["X"], np.zeros((PC.MOMENT_N, 1)), Gaussian(), [layer]), c


def test_the_moments_of_the_draws_are_the_closed_form_given_the_basis():
    model, c = _moment_model()
    fs = model.sample_functions(num_functions=PC.MOMENT_T, num_features=PC.MOMENT_L, seed=PC.MOMENT_SEED)
    F = fs(c["X"])[:, :, 0]
    rm, rc = PC.moment_ratios(F, fs.layers[0].Omega_host)
    print(f"device moments: mean {rm:.3g}, covariance {rc:.3g} standard errors")
    assert rm <= 5.0 and rc <= 5.0


def test_the_covariance_of_the_draws_is_the_joint_posterior_covariance_corrected_by_the_basis_term():
    """n = 32, T = 4096, one layer: predict_f_full_cov's covariance C is that of the joint draws; given the basis a pathwise draw has
    C + (K^ - K)(X, X) - B (K^ - K)(Z, X) - (K^ - K)(X, Z) B^T + B (K^ - K)(Z, Z) B^T, B = k(X, Z) Ku^-1, which is the closed form of
    tests/pathwise_reference.py:moments_given_basis minus the same form with K in K^'s place.  Within 5 standard errors; the float64
    twin of this configuration is held to 4 by tests/test_pathwise_reference_cpu.py on its 8 rows."""
    model, c = _moment_model()
    rng = np.random.default_rng(9)
    Xs = rng.uniform(-0.5, 3.5, size=(32, 2))
    fs = model.sample_functions(num_functions=4096, num_features=PC.MOMENT_L, seed=PC.MOMENT_SEED)
    F = fs(Xs)[:, :, 0]
    mean_j, var_j = model.predict_f_full_cov(Xs, 1)
    Cj = np.asarray(var_j)[0, :, :, 0]
    Om = fs.layers[0].Omega_host
    args = (c["kind"], Xs, Om, c["origin"], c["Z"], c["q_mu"], c["q_sqrt"], c["variance"], c["ls"], None, c["jitter"], False)
    mean_b, cov_b = PR.moments_given_basis(*args)
    # the same closed form with the exact kernel is the posterior covariance itself: the correction is their difference
    Lu = PR.cholesky(PR.ku(c["kind"], c["Z"], c["variance"], c["ls"], None, c["jitter"]))
    B = PR.solve_lower(Lu, PR.solve_lower(Lu, PR.kernel(c["kind"], c["Z"], Xs, c["variance"], c["ls"])), trans=True).T
    R = np.tril(np.asarray(c["q_sqrt"][0], dtype=PR.LD))
    exact = PR.kernel(c["kind"], Xs, Xs, c["variance"], c["ls"]) - B @ PR.kernel(c["kind"], c["Z"], Xs, c["variance"], c["ls"]) \
        + (B @ R) @ (B @ R).T
    want = Cj + (cov_b[0] - exact).astype(np.float64)
    assert np.max(np.abs(np.asarray(mean_j)[0, :, 0] - mean_b[:, 0].astype(np.float64))) <= 1e-6
    T = F.shape[0]
    se = np.sqrt((np.outer(np.diag(want), np.diag(want)) + want ** 2) / T)
    worst = float(np.max(np.abs(np.cov(F.T) - want) / se))
    print(f"joint covariance: {worst:.3g} standard errors")
    assert worst <= 5.0


def test_a_ku_that_is_not_positive_definite_raises_cholesky_error():
    from doubly_stochastic_dgp import _lib, settings
    model, _ = _moment_model()
    old = settings.jitter
    try:
        settings.jitter = -10.0
        with pytest.raises(_lib.CholeskyError):
            model.sample_functions(2, 16)
    finally:
        settings.jitter = old
    assert model.sample_functions(2, 16)(PC.moment_config()["X"]).shape == (2, PC.MOMENT_N, 1)
