"""-m gpu: held-out evaluation on the device (csrc/evaluate.hip; dsdgp_eval_mixture, dsdgp_model_evaluate, DGP_Base.evaluate) against
tests/evaluate_reference.py, the numpy / scipy restatement of demos/run_regression.py:108-123.

Primitive: random (mean, var, Y) at shapes on both sides of every boundary of the kernel — lanes per item (1 / 4 / 8 / 16: by the
item count at 4096, 8192 and 32768 and by S at 4, 8 and 16), the four-fold unrolled component loop (4 vs 5 components per lane), one
vs several workgroups with a ragged last one, the two-level in-workgroup sums (up to 32 outputs) vs the plain ones.
Tolerances: DESIGN 3's bound for primitives, rtol 1e-10 (atol 1e-13 for values that may cross zero); for the quadrature likelihoods'
log density the bound tests/test_gpu_likelihoods.py::test_var_exp_and_predict_primitives holds mode 1 to, rtol 1e-11 / atol 1e-13.
Sums over n rows get n times the absolute part.

Model level: DGP_Base.evaluate against the reference applied to the outputs of the existing path (_build_predict, the host likelihood,
numpy), with explicit draws and with device draws at the per-batch seeds of DGP_Base._draw_seed."""
import ctypes as C
import hashlib

import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import evaluate_reference as R
from tests.mixture_cases import NS, _build_case, _case, run_child

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-13)
TOL_QUAD_DENSITY = dict(rtol=1e-11, atol=1e-13)      # tests/test_gpu_likelihoods.py, predict_density_logmeanexp of the primitives
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


def _prim(ctx, kind, p0, p1, mean, var, Y, acc=None, accumulate=0, want_rows=True):
    """dsdgp_eval_mixture -> (acc (3, D) device tensor, rows (N, D, 3) numpy or None, return code)"""
    S, N, D = mean.shape
    m, v, y = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(Y)
    if acc is None:
        acc = ctx.empty(3, D)
    pad = 8
    rows = ctx.empty(N * D * 3 + pad) if want_rows else None
    if want_rows:
        with ctx.torch.cuda.stream(ctx.tstream):
            rows.fill_(-12345.25)
    rc = ctx.lib.dsdgp_eval_mixture(ctx.handle, kind, float(p0), float(p1), C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()),
                                    C.c_void_p(y.data_ptr()), N, S, D, C.c_void_p(rows.data_ptr() if want_rows else 0),
                                    C.c_void_p(acc.data_ptr()), accumulate)
    ctx.sync()
    if rc != 0 or not want_rows:
        return acc, None, rc
    host = rows.cpu().numpy()
    assert np.all(host[N * D * 3:] == -12345.25), "dsdgp_eval_mixture wrote past rows_out"
    return acc, host[:N * D * 3].reshape(N, D, 3), rc


def _check(acc, rows, ref_rows, ref_sums, n, density_tol=TOL):
    assert_allclose(rows[..., 0], ref_rows[..., 0], **TOL)
    assert_allclose(rows[..., 1], ref_rows[..., 1], **TOL)
    assert_allclose(rows[..., 2], ref_rows[..., 2], **density_tol)
    got = acc.cpu().numpy()
    assert_allclose(got[0], ref_sums[0], rtol=TOL["rtol"], atol=n * TOL["atol"])
    assert_allclose(got[1], ref_sums[1], rtol=density_tol["rtol"], atol=n * density_tol["atol"])
    assert np.array_equal(got[2], ref_sums[2])


def _gauss_inputs(n, DY, S, seed=0):
    rng = np.random.RandomState(1000 * seed + 7 * n + 3 * DY + S)
    return rng.randn(S, n, DY), rng.uniform(0.01, 1.5, size=(S, n, DY)), rng.randn(n, DY)


GAUSS_SHAPES = [
    # the issue's shapes
    (1, 1, 1), (37, 3, 3), (37, 1, 37), (1000, 1, 100), (4099, 2, 5),
    # lanes per item by S (few items: 16 lanes wanted): 1 | 4 | 8 | 16 at S = 4, 8, 16
    (37, 1, 4), (37, 1, 7), (37, 1, 8), (37, 1, 15), (37, 1, 16),
    # four-fold unrolled component loop, 16 lanes: exactly 4 per lane, 4 and 5, 5 per lane
    (37, 1, 64), (37, 1, 65), (37, 1, 80),
    # lanes per item by the item count: 16 | 8 at 4096, 8 | 4 at 8192, 4 | 1 at 32768 (the last also: one lane, 4 + 1 components)
    (4095, 1, 16), (4096, 1, 16), (8191, 1, 8), (8192, 1, 8), (32767, 1, 5), (32768, 1, 5), (16384, 2, 4),
    # in-workgroup sums: two levels up to 32 outputs, one above; a workgroup start that is no multiple of DY
    (5, 32, 3), (5, 33, 3), (3, 40, 2), (300, 3, 2), (23, 7, 20),
]


@pytest.mark.parametrize("n,DY,S", GAUSS_SHAPES)
def test_primitive_gaussian_shapes(ctx, n, DY, S):
    from doubly_stochastic_dgp import _lib
    mean, var, Y = _gauss_inputs(n, DY, S)
    s2 = 0.3
    ref_rows = R.mixture_rows(*R.gaussian_components(mean, var, Y, s2))
    acc, rows, rc = _prim(ctx, _lib.LIK_GAUSSIAN, s2, 1.0, mean, var, Y)
    assert rc == 0
    _check(acc, rows, ref_rows, R.sums(ref_rows, Y), n)
    if S == 1:      # one component: returned exactly
        assert np.array_equal(rows[..., 0], mean[0]) and np.array_equal(rows[..., 1], var[0] + s2)


@pytest.mark.parametrize("S", [5, 40])
def test_primitive_far_components_cost_nothing(ctx, S):
    """row 0: one component with var = 1e-8 centred on y, all others 40 standard deviations away (800 nats below it); row 1: the
    reverse — every component but one sits on y"""
    from doubly_stochastic_dgp import _lib
    rng = np.random.RandomState(3)
    s2 = 1e-12
    Y = rng.randn(2, 1)
    var = rng.uniform(0.5, 1.5, size=(S, 2, 1))
    mean = np.empty((S, 2, 1))
    mean[:, 0, 0] = Y[0, 0] + 40.0 * np.sqrt(var[:, 0, 0] + s2) * np.where(np.arange(S) % 2, 1.0, -1.0)
    mean[2, 0, 0], var[2, 0, 0] = Y[0, 0], 1e-8
    mean[:, 1, 0] = Y[1, 0]
    var[:, 1, 0] = 1e-8
    var[3, 1, 0] = 0.7
    mean[3, 1, 0] = Y[1, 0] - 40.0 * np.sqrt(0.7 + s2)
    ref_rows = R.mixture_rows(*R.gaussian_components(mean, var, Y, s2))
    acc, rows, rc = _prim(ctx, _lib.LIK_GAUSSIAN, s2, 1.0, mean, var, Y)
    assert rc == 0 and np.all(np.isfinite(rows))
    _check(acc, rows, ref_rows, R.sums(ref_rows, Y), 2)
    best = R.gaussian_components(mean, var, Y, s2)[0][2, 0, 0]
    assert_allclose(rows[0, 0, 2], best - np.log(S), rtol=1e-13)


def _lik_case(name, rng, n, DY):
    from doubly_stochastic_dgp.gpflow_compat import Bernoulli, Beta, Exponential, Gamma, Poisson, StudentT
    from tests.test_gpu_likelihoods import _targets
    if name == "bernoulli":
        return Bernoulli(), rng.choice([-1.0, 1.0], n * DY).reshape(n, DY)
    lik = {"poisson": Poisson(binsize=0.8), "exponential": Exponential(), "student_t": StudentT(1.3, 3.0), "gamma": Gamma(shape=2.2),
           "beta": Beta(scale=3.5)}[name]
    return lik, _targets(name, rng, n, DY)


@pytest.mark.parametrize("n,DY,S", [(37, 3, 3), (37, 2, 9)])
@pytest.mark.parametrize("name", ["bernoulli", "poisson", "exponential", "student_t", "gamma", "beta"])
def test_primitive_other_likelihoods(ctx, name, n, DY, S):
    from doubly_stochastic_dgp.utils import BroadcastingLikelihood
    rng = np.random.RandomState(5 + len(name))
    lik, Y = _lik_case(name, rng, n, DY)
    lik = BroadcastingLikelihood(lik)
    mean, var = 1.2 * rng.randn(S, n, DY), rng.uniform(1e-6, 2.0, size=(S, n, DY))
    ref_rows = R.mixture_rows(*R.host_components(lik, mean, var, Y))
    acc, rows, rc = _prim(ctx, *lik.mixture_args(), mean, var, Y)
    assert rc == 0
    _check(acc, rows, ref_rows, R.sums(ref_rows, Y), n, density_tol=TOL if name == "bernoulli" else TOL_QUAD_DENSITY)
    # the host wrapper goes the same way
    acc2, rows2 = lik.evaluate_mixture(mean, var, Y, rows=True)
    assert np.array_equal(acc2, acc.cpu().numpy()) and np.array_equal(rows2, rows)


@pytest.mark.parametrize("n,K,S", [(5, 10, 8), (37, 3, 3), (300, 4, 1), (37, 3, 20)])
def test_primitive_multiclass(ctx, n, K, S):
    from doubly_stochastic_dgp.gpflow_compat import MultiClass
    from doubly_stochastic_dgp.utils import BroadcastingLikelihood
    rng = np.random.RandomState(11 + K)
    lik = BroadcastingLikelihood(MultiClass(K))
    mean, var = 1.5 * rng.randn(S, n, K), rng.uniform(1e-3, 2.0, size=(S, n, K))
    if n > 30:      # a tie between two classes in every component of row 0: the lowest index wins
        mean[:, 0, :], var[:, 0, :] = -3.0, 0.5
        mean[:, 0, 1:3] = 1.0
    Y = rng.randint(0, K, size=(n, 1)).astype(np.float64)
    Y[0, 0] = 1.0
    ref_rows = R.mixture_rows(*R.host_components(lik, mean, var, Y))
    ref_sums = R.multiclass_sums(ref_rows, Y)
    acc, rows, rc = _prim(ctx, *lik.mixture_args(), mean, var, Y)
    assert rc == 0
    assert_allclose(rows, ref_rows, **TOL)
    got = acc.cpu().numpy()
    assert np.array_equal(got[0], ref_sums[0]) and np.array_equal(got[2], ref_sums[2]) and np.all(got[:, 1:] == 0.0)
    assert_allclose(got[1], ref_sums[1], rtol=TOL["rtol"], atol=n * TOL["atol"])
    if n > 30:
        assert rows[0, 1, 0] == rows[0, 2, 0] and np.argmax(rows[0, :, 0]) == 1      # the tie is exact, and row 0 counts as correct


@pytest.mark.parametrize("n,DY,S", [(37, 3, 3), (1000, 1, 100), (4099, 2, 5)])
def test_primitive_accumulates_and_repeats_bitwise(ctx, n, DY, S):
    from doubly_stochastic_dgp import _lib
    mean, var, Y = _gauss_inputs(n, DY, S, seed=1)
    s2 = 0.2
    ref_rows = R.mixture_rows(*R.gaussian_components(mean, var, Y, s2))
    ref = R.sums(ref_rows, Y)
    h = n // 2 + 1
    acc, _, rc = _prim(ctx, _lib.LIK_GAUSSIAN, s2, 1.0, np.ascontiguousarray(mean[:, :h]), np.ascontiguousarray(var[:, :h]), Y[:h],
                       want_rows=False)
    assert rc == 0
    acc, _, rc = _prim(ctx, _lib.LIK_GAUSSIAN, s2, 1.0, np.ascontiguousarray(mean[:, h:]), np.ascontiguousarray(var[:, h:]), Y[h:],
                       acc=acc, accumulate=1, want_rows=False)
    assert rc == 0
    got = acc.cpu().numpy()
    assert_allclose(got[0], ref[0], rtol=TOL["rtol"], atol=n * TOL["atol"])
    assert_allclose(got[1], ref[1], rtol=TOL["rtol"], atol=n * TOL["atol"])
    assert np.array_equal(got[2], ref[2])
    a1, r1, _ = _prim(ctx, _lib.LIK_GAUSSIAN, s2, 1.0, mean, var, Y)
    a2, r2, _ = _prim(ctx, _lib.LIK_GAUSSIAN, s2, 1.0, mean, var, Y)
    assert np.array_equal(a1.cpu().numpy(), a2.cpu().numpy()) and np.array_equal(r1, r2)


def test_primitive_rejects_what_it_does_not_cover(ctx):
    mean, var, Y = _gauss_inputs(4, 2, 2)
    assert _prim(ctx, 99, 1.0, 1.0, mean, var, Y)[2] == UNSUPPORTED
    assert b"not covered" in ctx.lib.dsdgp_last_error()
    m, v, _ = _gauss_inputs(4, 40, 2)
    assert _prim(ctx, 1, 1.0, 1.0, m, v, np.zeros((4, 1)))[2] == UNSUPPORTED          # MultiClass beyond 32 classes
    assert _prim(ctx, 0, 0.0, 1.0, mean, var, Y)[2] == -1                              # Gaussian variance must be positive
    assert _prim(ctx, 5, -1.0, 3.0, mean, var, Y)[2] == -1                             # StudentT scale


# ---------------------------------------------------------------- model level
MODELS = ["rbf", "matern_white", "bernoulli", "multiclass"]
_refs = {}


def _reference_from(model, Fm, Fv, Ys):
    from doubly_stochastic_dgp.gpflow_compat import MultiClass
    lik = model.likelihood
    if not lik.needs_broadcasting:
        rows = R.mixture_rows(*R.gaussian_components(Fm, Fv, Ys, float(lik.likelihood.variance.value)))
        return rows, R.sums(rows, Ys)
    rows = R.mixture_rows(*R.host_components(lik, Fm, Fv, Ys))
    return rows, (R.multiclass_sums(rows, Ys) if isinstance(lik.likelihood, MultiClass) else R.sums(rows, Ys))


def _reference(name, S):
    """the parent path: _build_predict on all rows at once, the host likelihood, numpy — computed once per (model, S)"""
    if (name, S) not in _refs:
        model, Xs, Ys, zs = _case(name)
        Fm, Fv = model._build_predict(Xs, S=S, zs=[z[:S] for z in zs])
        _refs[name, S] = _reference_from(model, Fm, Fv, Ys)
    return _refs[name, S]


def _check_scores(out, rows, sums, name, Y_std=1.0):
    want = R.scores(sums, Y_std=Y_std, gaussian=name in ("rbf", "matern_white"), multiclass=name == "multiclass")
    assert_allclose(out["rows"], rows, **TOL)
    assert out["n"] == NS
    assert set(want) <= set(out)
    for k, v in want.items():
        if k == "error_rate":
            assert out[k] == v
        else:
            assert_allclose(out[k], v, **TOL)


@pytest.mark.parametrize("S", [1, 3, 37])
@pytest.mark.parametrize("batch_size", [16, 37, 1000])
@pytest.mark.parametrize("name", MODELS)
def test_evaluate_matches_the_parent_path(name, batch_size, S):
    model, Xs, Ys, zs = _case(name)
    rows, sums = _reference(name, S)
    out = model.evaluate(Xs, Ys, S, batch_size=batch_size, zs=[z[:S] for z in zs], return_rows=True)
    _check_scores(out, rows, sums, name)


def test_evaluate_takes_device_tensors_and_broadcast_draws():
    model, Xs, Ys, zs = _case("rbf")
    ctx = model.engine().ctx
    S = 3
    zb = [zs[0][:S, :1], zs[1][:1]]                      # one draw shared by all rows / by all samples
    Fm, Fv = model._build_predict(Xs, S=S, zs=zb)
    rows, sums = _reference_from(model, Fm, Fv, Ys)
    out = model.evaluate(ctx.to_device(Xs), ctx.to_device(Ys), S, batch_size=16, zs=[ctx.to_device(z) for z in zb], return_rows=True)
    _check_scores(out, rows, sums, "rbf")


@pytest.mark.parametrize("name", ["rbf", "multiclass"])
def test_evaluate_device_draws_use_one_seed_per_batch(name):
    """zs = None: batch k of the call draws under the k-th _draw_seed() after the call's start (world = 1: seed + k + 1) — the formula
    tests/test_gpu_device_draws.py pins; _build_predict on the same rows under the same seed is the parent path"""
    model, Xs, Ys, _ = _case(name)
    S, bs = 3, 16
    s0 = model._seed
    out = model.evaluate(Xs, Ys, S, batch_size=bs, return_rows=True)
    assert model._seed == s0 + 3
    Fm, Fv = [], []
    for k, a in enumerate(range(0, NS, bs)):
        model._seed = s0 + k
        m, v = model._build_predict(Xs[a:a + bs], S=S)
        Fm.append(m); Fv.append(v)
    model._seed = s0 + 3
    rows, sums = _reference_from(model, np.concatenate(Fm, 1), np.concatenate(Fv, 1), Ys)
    _check_scores(out, rows, sums, name)


def test_evaluate_y_std_reproduces_run_regression():
    """demos/run_regression.py:109-123 literally on predict_y outputs, batch by batch, with Y_std = 2.5"""
    model, Xs, Ys, zs = _case("matern_white")
    S, bs, Y_std = 3, 16, 2.5
    means, vars_ = [], []
    for a in range(0, NS, bs):
        Fm, Fv = model._build_predict(Xs[a:a + bs], S=S, zs=[z[:S, a:a + bs] for z in zs])
        m, v = model.likelihood.predict_mean_and_var(Fm, Fv)
        means.append(m); vars_.append(v)
    err, nll = R.run_regression_scores(np.concatenate(means, 1), np.concatenate(vars_, 1), Ys, Y_std)
    out = model.evaluate(Xs, Ys, S, batch_size=bs, Y_std=Y_std, zs=[z[:S] for z in zs])
    assert_allclose(out["rmse"], err, **TOL)
    assert_allclose(out["log_density"], nll, **TOL)
    assert "rows" not in out


_CHILD = r"""
import hashlib, json, sys
sys.path[:0] = sys.argv[1:3]
import numpy as np
from tests import test_gpu_evaluate as T
print(json.dumps(T._bits_of_one_run()))
"""


def _bits_of_one_run():
    """evaluate on the RBF model with explicit draws: digests of its rows and scores, and whether they equal, bit for bit, the
    primitive applied to this process's own _build_predict outputs (one batch: same rows in the workspace and in the copy)"""
    from doubly_stochastic_dgp.engine import Context
    model, Xs, Ys, zs = _build_case("rbf")
    S = 3
    z = [q[:S] for q in zs]
    out = model.evaluate(Xs, Ys, S, batch_size=16, zs=z, return_rows=True)
    one = model.evaluate(Xs, Ys, S, batch_size=1000, zs=z, return_rows=True)
    Fm, Fv = model._build_predict(Xs, S=S, zs=z)
    acc, rows = model.likelihood.evaluate_mixture(Fm, Fv, Ys, rows=True)
    want = R.scores(acc)
    same = bool(np.array_equal(rows, one["rows"]) and want["rmse"] == one["rmse"] and want["log_density"] == one["log_density"])
    return {"forward": hashlib.sha256(Fm.tobytes() + Fv.tobytes()).hexdigest(),
            "rows": hashlib.sha256(out["rows"].tobytes()).hexdigest(), "rmse": float(out["rmse"]).hex(),
            "log_density": float(out["log_density"]).hex(), "same_as_primitive": same,
            "launches": int(Context.get().lib.dsdgp_launch_count())}


@pytest.fixture(scope="module")
def default_bits():
    return run_child(_CHILD, {})


@pytest.mark.parametrize("env", [{"DSDGP_NO_OVERLAP": "1"}, {"DSDGP_FORCE": "gemm_mp=16"}], ids=["no_overlap", "gemm"])
def test_evaluate_bits_do_not_depend_on_the_forward_path(default_bits, env):
    """Each switch in a fresh child process (both are read when the device model is created).  The reduction adds no dependence on the
    path of its own: in every process evaluate equals, bit for bit, the primitive applied to that process's _build_predict outputs, and
    two processes whose forward passes wrote the same bits report the same bits.  The single-stream schedule runs the same kernels as
    the default, so there the bits must agree outright; the GEMM-formulated chains sum in another order
    (tests/test_gpu_gemm_path.py asserts that their predictions differ from the chains' in the last bits), so their scores are held to
    that file's chain-against-GEMM bound instead, rtol 1e-8."""
    got = run_child(_CHILD, env)
    print("default", default_bits, "\n", env, got)
    assert default_bits["same_as_primitive"] and got["same_as_primitive"]
    if "DSDGP_NO_OVERLAP" in env:
        assert got["forward"] == default_bits["forward"]
    if got["forward"] == default_bits["forward"]:
        for k in ("rows", "rmse", "log_density"):
            assert got[k] == default_bits[k], k
    else:
        for k in ("rmse", "log_density"):
            assert_allclose(float.fromhex(got[k]), float.fromhex(default_bits[k]), rtol=1e-8)


def test_evaluate_fails_loudly_outside_its_scope():
    from doubly_stochastic_dgp import _lib
    model, Xs, Ys, zs = _case("bernoulli")
    with pytest.raises(TypeError):
        model.evaluate(Xs, Ys, 3, full_cov=True)
    with pytest.raises(ValueError):
        model.evaluate(Xs, Ys, 3, Y_std=2.5)              # only a Gaussian density rescales
    with pytest.raises(ValueError):
        model.evaluate(Xs, Ys[:, :1], 3)                  # targets of the wrong width never reach the kernel
    with pytest.raises(ValueError):
        model.evaluate(Xs, Ys[:-1], 3)
    mc = _case("multiclass")
    with pytest.raises(ValueError):
        mc[0].evaluate(mc[1], mc[2] + 0.5, 3)             # labels must be integers in [0, K)
    # a model carrying quadrature sample weights (DGP_Quad) is not an unweighted mixture
    eng = model.engine()
    eng.set_sample_weights(eng.ctx.to_device(np.full(3, 1.0 / 3.0)))
    try:
        with pytest.raises(_lib.DsdgpError, match="-4"):
            model.evaluate(Xs, Ys, 3)
    finally:
        eng.set_sample_weights(None)
    assert np.isfinite(model.evaluate(Xs, Ys, 3)["log_density"])
