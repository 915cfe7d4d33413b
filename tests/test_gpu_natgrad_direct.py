"""dsdgp_model_natgrad_step driven directly: a chosen (q_mu, q_sqrt), a SYNTHETIC gradient written into the device gradient buffer, one
step, and the result compared with the step in extended precision (tests/natgrad_reference.py) — on every factorisation path the step
has (tests/natgrad_cases.py), so that an error in the step is not mixed with gradient error and q_sqrt is a dense triangle at every size.

Per case (eps = 2^-52, n = M): the four scaled measures fwd_T, fwd_m, congruence, mean_residual of natgrad_reference, each at most
factor_reference.device_bar(the worse of the two float64 CPU comparators on the same input) = 8 x that value, never below 1.0; and the
exact structure of q_sqrt+ (+0.0 above the diagonal, positive diagonal, finite).
Further: the model's own gradient at M = 180 / 300 (the question tests/test_gpu_round6.py left open), two steps in a row, the ELBO after
the step against the oracle at the reference's parameters, and a refused step (A indefinite: CholeskyError, nothing moved).

Set DSDGP_NATGRAD_PROFILE=<file> to get every measured device and CPU value as one table (profiles/natgrad_direct_errors.md).
111 cases, about half a minute on an MI355X with 16 host cores (the extended-precision steps run once, in worker processes)."""
import os
import time

import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import dgp_oracle as O, model as OM
from tests import natgrad_reference as NG
from tests.helpers import kern_spec, make_case
from tests.natgrad_cases import CASES, REFUSED_M, TWO_STEP_M, UNIFORM_BIG_M, case_id, case_inputs

pytestmark = pytest.mark.gpu

N, D_IN = 16, 3


def padded(M):
    from doubly_stochastic_dgp.engine import padded_M
    return padded_M(M)


# ------------------------------------------------------------------------------------------------ the model and the step
_MODEL = {}


def tiny_model(M, D_outs, white, plain, monkeypatch):
    """(spec, state, model, X, Y, zs) on N = 16 rows, S = 1: one layer per entry of D_outs (inner layers have D_in = 3 outputs, the
    last one Y's), all on the same M inducing points.  The last model is kept: consecutive cases of the table share it."""
    monkeypatch.delenv("DSDGP_FORCE", raising=False)
    if plain:
        monkeypatch.setenv("DSDGP_CHOL_LOOKAHEAD", "0")        # read when the plan is built: a fresh model
    else:
        monkeypatch.delenv("DSDGP_CHOL_LOOKAHEAD", raising=False)
    key = (M, tuple(D_outs), white, plain)
    if key not in _MODEL:
        _MODEL.clear()
        rng = np.random.RandomState(M + 7 * len(D_outs))
        X, Y = rng.randn(N, D_IN), rng.randn(N, D_outs[-1])
        Z = 2.0 * rng.randn(M, D_IN)
        specs = [kern_spec("rbf", D_IN, 1.0, 1.0)] * len(D_outs)
        spec, state, model = make_case(X, Y, Z, specs, white=white, S=1, seed=M)
        assert [l.num_outputs for l in model.layers] == list(D_outs)
        zs = [rng.randn(1, N, d) for d in D_outs]
        _MODEL[key] = (spec, state, model, X, Y, zs)
    return _MODEL[key]


def _segment(eng, param):
    for p, off, cnt, kind in eng.entries:
        if p is param:
            return off, cnt
    raise KeyError("parameter not in the engine's layout")


def inject_gradient(eng, layer, g_mu, g_sqrt):
    """overwrite the (M, D_out) and (D_out, M, M) segments of the device gradient of the last evaluation"""
    torch = eng.ctx.torch
    eng.ctx.sync()
    for p, val in ((layer.q_mu, g_mu), (layer.q_sqrt, g_sqrt)):
        off, cnt = _segment(eng, p)
        val = np.ascontiguousarray(val, dtype=np.float64)
        assert val.size == cnt and val.shape == tuple(p.shape)
        eng.grad[off:off + cnt].copy_(torch.as_tensor(val.ravel()))
    torch.cuda.synchronize()


def device_step(model, X, Y, zs, l, q_mu, q_sqrt, g_mu, g_sqrt, gamma, check=True):
    """set layer l's (q_mu, q_sqrt), evaluate once with a gradient (uploads the parameters, prepares Tp), replace that layer's gradient
    by the synthetic one, step -> (q_mu+, q_sqrt+) read back through the Parameters"""
    layer = model.layers[l]
    layer.q_mu = q_mu
    layer.q_sqrt = q_sqrt
    model._build_likelihood(X, Y, zs=zs, with_grad=True)
    eng = model.engine()
    inject_gradient(eng, layer, g_mu, g_sqrt)
    eng.natgrad_step(l, gamma, check=check)
    eng.sync_to_host()
    return np.array(layer.q_mu.value), np.array(layer.q_sqrt.value)


# ------------------------------------------------------------------------------------------------ the profile table
_ROWS = []
_REAL = []


@pytest.fixture(scope="module", autouse=True)
def profile_table():
    t0 = time.time()
    yield
    path = os.environ.get("DSDGP_NATGRAD_PROFILE")
    if not path or not _ROWS:
        return
    hdr = ["case", "path", "white", "n", "Mp", "D_out", "gamma"]
    for k in NG.MEASURES:
        hdr += [f"{k} dev", f"{k} oracle", f"{k} reversed", f"{k} bar"]
    with open(path, "w") as f:
        f.write("# One natural-gradient step on the device against the step in extended precision (tests/test_gpu_natgrad_direct.py)\n\n"
                "Scaled measures as defined in tests/natgrad_reference.py (units of n eps, the worst output d); `oracle` = oracle.dgp_oracle.natgrad_step,\n"
                "`reversed` = the device's algorithm in LAPACK float64, both on the same input; `bar` = 8 x the larger of the two, never below 1.0\n"
                "(+ 1.0 for the float64 products of the measure from n = 1024 on).\n\n")
        f.write("| " + " | ".join(hdr) + " |\n|" + "---|" * len(hdr) + "\n")
        for r in _ROWS:
            f.write("| " + " | ".join(r) + " |\n")
        if _REAL:
            f.write("\n## The model's own gradient: the device against the float64 oracle in the form tests/test_gpu_round6.py asserts\n\n"
                    "| M | layers | white | cond(A) | max abs(dev - oracle) / (1e-8 + 1e-6 abs(oracle)) |\n|---|---|---|---|---|\n")
            for r in _REAL:
                f.write("| " + " | ".join(r) + " |\n")
        f.write(f"\n{len(_ROWS)} steps, {time.time() - t0:.0f} s for the module.\n")


def check_step(name, path, white, M, gamma, got_mu, got_sq, inputs):
    """structure + the four measures against the bars; one row of the table"""
    NG.check_structure(got_sq, name)
    assert np.all(np.isfinite(got_mu)), f"{name}: NaN / Inf in q_mu+"
    ref, cpu = NG.cpu_measures(*inputs, gamma)
    dev = NG.measures(got_mu, got_sq, ref)
    bars = NG.bars(cpu, M)
    row = [name, path, str(int(white)), str(M), str(padded(M)), str(got_mu.shape[1]), f"{gamma:g}"]
    for k in NG.MEASURES:
        row += [f"{dev[k]:.3g}", f"{cpu['oracle'][k]:.3g}", f"{cpu['reversed'][k]:.3g}", f"{bars[k]:.3g}"]
    print("NATGRAD_DIRECT | " + " | ".join(row))
    _ROWS.append(row)
    for k in NG.MEASURES:
        assert dev[k] <= bars[k], f"{name}: {k} {dev[k]:.3g} > bar {bars[k]:.3g} (oracle {cpu['oracle'][k]:.3g}, reversed {cpu['reversed'][k]:.3g})"
    return ref


@pytest.fixture(scope="module")
def references():
    """the longdouble step and both comparators of every case of the table, once, in worker processes"""
    NG.prefill([case_inputs(c.t_family, c.M, c.D_out, c.g_family) + (c.gamma,) for c in CASES])


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_step_on_a_synthetic_gradient(monkeypatch, references, case):
    c = case
    spec, state, model, X, Y, zs = tiny_model(c.M, (c.D_out,), c.white, c.plain, monkeypatch)
    inputs = case_inputs(c.t_family, c.M, c.D_out, c.g_family)
    mu, sq = device_step(model, X, Y, zs, 0, *inputs, c.gamma)
    ref = check_step(case_id(c), c.path, c.white, c.M, c.gamma, mu, sq, inputs)
    if c.eval_after:
        # the ELBO on the stepped parameters (Ku unchanged: its factor is kept; q moved) against the oracle at the REFERENCE's parameters
        state2 = dict(state)
        state2["l0.q_mu"], state2["l0.q_sqrt"] = np.asarray(ref[0], dtype=np.float64), np.asarray(ref[1], dtype=np.float64)
        assert_allclose(model.compute_log_likelihood(X, Y, zs=zs), OM.elbo(spec, state2, X, Y, zs, 1), rtol=1e-8)


@pytest.mark.parametrize("tf", ["dense", "init_prior"])
def test_two_layers_sharing_one_batched_sequence(monkeypatch, tf):
    """M = 192 on both layers (uniform_big): a step on layer 0 (D_out = 3, an inner layer), then on layer 1 (D_out = 2), each on its own
    synthetic gradient; then the ELBO against the oracle at the reference's parameters of both layers"""
    M = UNIFORM_BIG_M
    spec, state, model, X, Y, zs = tiny_model(M, (3, 2), False, False, monkeypatch)
    state2 = dict(state)
    for l, (D_out, gf) in enumerate(((3, "generic"), (2, "quad"))):
        inputs = case_inputs(tf, M, D_out, gf, seed=l + 1)
        mu, sq = device_step(model, X, Y, zs, l, *inputs, 0.1)
        ref = check_step(f"uniform_big-M{M}-layer{l}-D{D_out}-{tf}-{gf}", "look-ahead x2", False, M, 0.1, mu, sq, inputs)
        state2[f"l{l}.q_mu"], state2[f"l{l}.q_sqrt"] = np.asarray(ref[0], dtype=np.float64), np.asarray(ref[1], dtype=np.float64)
    assert_allclose(model.compute_log_likelihood(X, Y, zs=zs), OM.elbo(spec, state2, X, Y, zs, 1), rtol=1e-8)


@pytest.mark.parametrize("M", TWO_STEP_M)
def test_two_steps_in_a_row(monkeypatch, M):
    """a second step on the first one's result (prepare_async runs again for Tp), a second synthetic gradient injected in between.
    The device continues from ITS first result, the reference from the first reference result (rounded to float64): the second result
    is held to two reference steps, within the second step's bars — the first step's error, itself within its bar, passes through a
    well-conditioned step (`dense`) without growing."""
    spec, state, model, X, Y, zs = tiny_model(M, (2,), False, False, monkeypatch)
    in1 = case_inputs("dense", M, 2, "generic")
    mu1, sq1 = device_step(model, X, Y, zs, 0, *in1, 0.1)
    ref1 = check_step(f"two-steps-M{M}-first", "two steps", False, M, 0.1, mu1, sq1, in1)
    r_mu, r_sq = np.asarray(ref1[0], dtype=np.float64), np.asarray(ref1[1], dtype=np.float64)
    g_mu, g_sqrt = NG.g_family("quad", r_mu, r_sq, seed=3)
    # the device continues from ITS parameters (nothing is set from the host): evaluate, inject, step
    layer, eng = model.layers[0], model.engine()
    model._build_likelihood(X, Y, zs=zs, with_grad=True)
    inject_gradient(eng, layer, g_mu, g_sqrt)
    eng.natgrad_step(0, 0.1)
    eng.sync_to_host()
    mu2, sq2 = np.array(layer.q_mu.value), np.array(layer.q_sqrt.value)
    check_step(f"two-steps-M{M}-second", "two steps", False, M, 0.1, mu2, sq2, (r_mu, r_sq, g_mu, g_sqrt))


# ------------------------------------------------------------------------------------------------ the model's own gradient
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("M,L", [(180, 1), (300, 3), (448, 1)])
def test_step_on_the_models_own_gradient(M, L, white):
    """tests/test_gpu_round6.py::test_lookahead_blocked_cholesky_in_the_model_against_the_oracle with make_case(randomize=True) kept for
    the natural-gradient step: same data shapes, the device's own gradient (read back and fed to the references), a step on the last
    layer, the same bars as every synthetic case.  Also printed: the largest error relative to the oracle's float64 step in the form
    that test asserts (|dev - oracle| <= 1e-8 + 1e-6 |oracle| entrywise)."""
    rng = np.random.RandomState(M + L)
    n, D, S = 24, 3, 2
    X, Y = rng.randn(n, D), rng.randn(n, 2)
    Z = rng.randn(M, D) * 2.0
    specs = [kern_spec("rbf", D, 1.0, 1.0)] * (L - 1) + [kern_spec("matern52", D, 1.3, 0.9)]
    spec, state, model = make_case(X, Y, Z, specs, white=white, S=S, num_data=500)
    zs = [rng.randn(S, n, D) for _ in range(L - 1)] + [rng.randn(S, n, 2)]
    model._build_likelihood(X, Y, zs=zs, with_grad=True)
    eng = model.engine()
    g = eng.gradient_dict()
    last = f"l{L - 1}"
    inputs = (state[last + ".q_mu"], np.tril(state[last + ".q_sqrt"]), g[last + ".q_mu"], np.tril(g[last + ".q_sqrt"]))
    eng.natgrad_step(L - 1, 0.1)
    eng.sync_to_host()
    lay = model.layers[-1]
    mu, sq = np.array(lay.q_mu.value), np.array(lay.q_sqrt.value)
    o_mu, o_sq = O.natgrad_step(*inputs, 0.1)
    worst = max(float(np.max(np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b)))) for a, b in ((mu, o_mu), (sq, o_sq)))
    cond = max(float(np.linalg.cond(np.asarray(A, dtype=np.float64))) for A in NG.step_ld(*inputs, 0.1)[2])
    _REAL.append([str(M), str(L), str(int(white)), f"{cond:.3g}", f"{worst:.3g}"])
    print("NATGRAD_REAL | " + " | ".join(_REAL[-1]))
    check_step(f"own-gradient-M{M}-L{L}" + ("-white" if white else ""), "look-ahead, model gradient", white, M, 0.1, mu, sq, inputs)


# ------------------------------------------------------------------------------------------------ a refused step
@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("M", REFUSED_M)
def test_refused_step_moves_nothing(monkeypatch, M, check):
    """quad with W replaced by -5 W at gamma = 1: A = S^-1 - 5 W is indefinite (asserted on the CPU first), the factorisation reports a
    failing pivot — the defined error path of dsdgp_potrf.  [UPSTREAM] tf.cholesky raises and no variable is assigned: here
    CholeskyError (check=True; check=False returns silently), and the layer's q_mu / q_sqrt on the host and in the device's theta are
    bit for bit what they were, as is the next evaluation.  (Before k_ng_mu / k_ng_write tested the factorisation's info on the
    device, all four cases failed at the comparison of theta: the write-back ran ahead of the host's look at info, and the host
    Parameters kept the old values while the device evaluated on the overwritten ones.)"""
    from doubly_stochastic_dgp import _lib
    q_mu, q_sqrt, g_mu, g_sqrt = case_inputs("dense", M, 2, "quad", w_scale=-5.0)
    for A in NG.assemble_ld(q_mu, q_sqrt, g_mu, g_sqrt, 1.0):
        ev = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
        assert ev[0] < 0 < ev[-1]
    spec, state, model, X, Y, zs = tiny_model(M, (2,), False, False, monkeypatch)
    layer, eng = model.layers[0], model.engine()
    layer.q_mu = q_mu
    layer.q_sqrt = q_sqrt
    before = model._build_likelihood(X, Y, zs=zs, with_grad=True)
    eng.ctx.sync()
    theta0 = eng.theta.cpu().numpy().copy()
    inject_gradient(eng, layer, g_mu, g_sqrt)
    if check:
        with pytest.raises(_lib.CholeskyError):
            eng.natgrad_step(0, 1.0)
    else:
        eng.natgrad_step(0, 1.0, check=False)
    eng.ctx.sync()
    theta1 = eng.theta.cpu().numpy()
    assert np.array_equal(theta0.view(np.uint64), theta1.view(np.uint64)), "the refused step wrote into the device's theta"
    eng.sync_to_host()
    assert np.array_equal(np.asarray(layer.q_mu.value).view(np.uint64), q_mu.view(np.uint64))
    assert np.array_equal(np.asarray(layer.q_sqrt.value).view(np.uint64), q_sqrt.view(np.uint64))
    after = model._build_likelihood(X, Y, zs=zs, with_grad=True)
    assert after == before
    # and the model still steps: the benign gradient of the same family
    inputs = case_inputs("dense", M, 2, "quad")
    mu, sq = device_step(model, X, Y, zs, 0, *inputs, 0.1)
    NG.check_structure(sq, f"after a refused step, M={M}")
    ref, cpu = NG.cpu_measures(*inputs, 0.1)
    dev, bars = NG.measures(mu, sq, ref), NG.bars(cpu, M)
    for k in NG.MEASURES:
        assert dev[k] <= bars[k], (k, dev[k], bars[k])
