"""-m gpu: the N(0, 1) draws the device makes by itself, pinned exactly.

Real training and prediction never pass `zs`: the inner layers' draws come from one of three places, picked by model shape and
schedule (model_schedule.hpp elbo_impl / forward_layers):

  head    spare block columns of the fused head launch (HeadRand; every layer Mp <= 128 and D_in <= 16, DSDGP_FORCE head = 1)
  side    k_randn on the side stream while Ku is factorised (head off, two-stream overlap on: n S Mp >= overlap_min)
  inline  k_randn in front of each layer's forward chain (head off, DSDGP_NO_OVERLAP=1; predictions always; the last layer always)

and sample_from_conditional(z=None) / the full_cov propagation draw through Engine.randn (seed 0x5eed, stream 2^32 | k).

1. dsdgp_randn equals the numpy restatement of the stream (oracle/philox.py) to Box-Muller rounding, over several grid-stride
   passes, with high seed / stream words, and writes nothing past `count`.
2. Every sampling entry point, called with device draws at a known seed, equals the same entry called with explicit draws
   dsdgp_randn(seed, l, S n D_out[l]) BIT FOR BIT (all reductions on the path are fixed-order); the launch counter shows which
   draw path ran (the head path adds no k_randn launch, the other two one per sampled layer).  Once per entry the explicit draws
   also go through the CPU oracle.
3. Eight consecutive device-drawn minibatch steps equal their replay with explicit draws after every step (a stale or raced
   draw buffer shows up from the second step on), and no two (layer, step) draw blocks coincide.
"""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import dgp_oracle as O
from oracle import model as OM
from oracle.philox import randn_reference
from tests.helpers import kern_spec, make_case, product_kernel

pytestmark = pytest.mark.gpu

# DSDGP_FORCE / DSDGP_NO_OVERLAP (both read when the device model is created; DSDGP_NO_OVERLAP also per call)
MODES = {"head": (None, "0"), "side": ("head=0,overlap_min=1", "0"), "inline": ("head=0", "1")}
ENGINE_SEED = 0x5eed


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


def _set_mode(monkeypatch, mode):
    force, no_overlap = MODES[mode]
    if force is None:
        monkeypatch.delenv("DSDGP_FORCE", raising=False)
    else:
        monkeypatch.setenv("DSDGP_FORCE", force)
    monkeypatch.setenv("DSDGP_NO_OVERLAP", no_overlap)


def _launches(ctx):
    return int(ctx.lib.dsdgp_launch_count())


def _device_randn(ctx, seed, stream, count, pad=8):
    """dsdgp_randn into a buffer of count + pad entries pre-filled with a sentinel; returns (draws, the pad afterwards)"""
    from doubly_stochastic_dgp import _lib
    buf = ctx.empty(count + pad)
    with ctx.torch.cuda.stream(ctx.tstream):
        buf.fill_(-12345.25)
    _lib.check(ctx.lib.dsdgp_randn(ctx.handle, C.c_uint64(seed), C.c_uint64(stream), count, C.c_void_p(buf.data_ptr())))
    ctx.sync()
    host = buf.cpu().numpy()
    return host[:count].copy(), host[count:].copy()


def _draw(ctx, seed, stream, shape):
    z, _ = _device_randn(ctx, seed, stream, int(np.prod(shape)))
    return z.reshape(shape)


# ---------------------------------------------------------------- 1. dsdgp_randn against the reference stream
@pytest.mark.parametrize("seed,stream", [(7, 3), (0xA5A5_0001_DEAD_BEEF, (5 << 32) | 2)])
@pytest.mark.parametrize("count", [1, 2, 3, 255, 257, (1 << 20) - 1, (1 << 20) + 1, (1 << 21) + 3])
def test_randn_matches_reference(ctx, seed, stream, count):
    """counts past 2^20 take more than one grid-stride pass of k_randn (its grid is capped at 2048 x 256 threads x 2 values)"""
    z, pad = _device_randn(ctx, seed, stream, count)
    ref = randn_reference(seed, stream, count)
    err = np.abs(z - ref) / np.maximum(1.0, np.abs(ref))
    worst = int(np.argmax(err))
    assert err[worst] <= 1e-13, (worst, z[worst], ref[worst])
    assert np.all(pad == -12345.25), "dsdgp_randn wrote past count"


# ---------------------------------------------------------------- model shapes
def _input_prop_model(minibatch_size=None):
    """3 layers with input propagation (layer_initializations.py:55-79): D_out 3, 2, 1, input_prop_dim 2, 2, None"""
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.dgp import DGP_Base
    from doubly_stochastic_dgp.gpflow_compat import Gaussian
    from doubly_stochastic_dgp.layer_initializations import init_layers_input_prop
    rng = np.random.RandomState(31)
    N, D, M, S = 40, 2, 14, 3
    X, Y = rng.randn(N, D), rng.randn(N, 1)
    Z = X[:M] + 0.01 * rng.randn(M, D)
    specs = [kern_spec("rbf", 2, 1.3, 0.9), kern_spec("matern52", 5, 0.8, 1.4), kern_spec("rbf", 4, 1.1, 1.2, ARD=True)]
    np.random.seed(5)
    pads = [np.random.randn(M, k["input_dim"] - D) for k in specs]
    lds = O.init_layers_input_prop(X, Y, Z, specs, pads)
    for l in lds:
        l["q_mu"] = 0.3 * rng.randn(*l["q_mu"].shape)
        l["q_sqrt"] = l["q_sqrt"] * 0.7 + 0.05 * np.tril(rng.randn(*l["q_sqrt"].shape))
    sl, state = OM.state_from_layers(lds, lik_variance=0.2)
    spec = dict(jitter=1e-6, white=False, likelihood="gaussian", layers=sl, num_classes=None)
    np.random.seed(5)
    with settings.temp_jitter(1e-6):
        layers = init_layers_input_prop(X, Y, Z, [product_kernel(k) for k in specs])
        model = DGP_Base(X, Y, Gaussian(variance=0.2), layers, num_samples=S, num_data=123, minibatch_size=minibatch_size)
    for l, layer in zip(lds, model.layers):
        layer.q_mu = l["q_mu"]
        layer.q_sqrt = l["q_sqrt"]
    assert [l.input_prop_dim for l in model.layers] == [2, 2, None]
    return X, Y, spec, state, model, S, 123


def _case(name, minibatch_size=None):
    """(X, Y, spec, state, model, S, num_data): a fresh model with the same parameters on every call"""
    if name == "input_prop":
        return _input_prop_model(minibatch_size)
    if name == "big":
        # Mp > 128: the head launch is ineligible; n S Mp = 300 * 8 * 160 >= 2^18, so the default schedule overlaps
        rng = np.random.RandomState(17)
        N, D, M, S = 300, 4, 150, 8
        X, Y = rng.randn(N, D), rng.randn(N, 1)
        Z = X[:M] + 0.05 * rng.randn(M, D)
        specs = [kern_spec("rbf", D, 1.0, 1.2), kern_spec("matern52", D, 0.9, 1.1), kern_spec("rbf", D, 1.1, 1.0)]
        spec, state, model = make_case(X, Y, Z, specs, S=S, num_data=1000, minibatch_size=minibatch_size)
        return X, Y, spec, state, model, S, 1000
    # "three", "three_white", "mixed": 3 layers of D_out 3, 5, 1 (S n D_out = 333, 555, 111: odd)
    rng = np.random.RandomState(3)
    N, S = 37, 3
    X, Y = rng.randn(N, 2), rng.randn(N, 1)
    Z = X[:20] + 0.01 * rng.randn(20, 2)
    specs = [kern_spec("rbf", 2, 1.1, 0.9), kern_spec("matern52", 3, 0.8, 1.2), kern_spec("rbf", 5, 1.0, 1.1)]
    spec, state, model = make_case(X, Y, Z, specs, white=(name == "three_white"), S=S, num_data=100, minibatch_size=minibatch_size)
    return X, Y, spec, state, model, S, 100


def _head_eligible(model):
    return all(l.feature.Z.shape[0] <= 128 and l.feature.Z.shape[1] <= 16 for l in model.layers)


def _fixed_zs(name, model, S, n):
    """the caller's explicit draws of the device-drawn call: layer 0 in the mixed case, nothing otherwise"""
    if name != "mixed":
        return None
    rng = np.random.RandomState(123)
    return [rng.randn(S, n, model.layers[0].num_outputs), None, None]


def _replay_zs(ctx, model, seed, S, n, fixed, layers):
    """fixed draws where the caller gave them, dsdgp_randn(seed, l, S n D_out) for the layers in `layers`, None elsewhere"""
    out = []
    for l, layer in enumerate(model.layers):
        if fixed is not None and fixed[l] is not None:
            out.append(fixed[l])
        elif l in layers:
            out.append(_draw(ctx, seed, l, (S, n, layer.num_outputs)))
        else:
            out.append(None)
    return out


def _oracle_zs(zs):
    return [np.zeros((1, 1, 1)) if z is None else z for z in zs]


def _state_of(eng, elbo=None):
    eng.ctx.sync()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in ("theta", "grad", "adam_m", "adam_v", "out4")}
    if elbo is not None:
        out["elbo"] = np.array([elbo])
    return out


def _assert_bitwise(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert np.all(np.isfinite(want[k])), (what, k)
        if not np.array_equal(got[k], want[k]):
            d = np.abs(np.asarray(got[k], float) - np.asarray(want[k], float))
            raise AssertionError(f"{what}: {k} differs from the replay with explicit draws at {int(np.count_nonzero(d))} of "
                                 f"{d.size} entries (max |diff| {d.max():.3e})")


# ---------------------------------------------------------------- 2. ELBO / training entries x the three draw paths
TRAIN_ENTRIES = ["elbo", "elbo_grad", "train_step", "train_step_minibatch"]
SHAPES = ["three", "three_white", "input_prop", "big", "mixed"]


def _call(entry, model, X, Y, zs):
    eng = model.engine()
    if entry == "elbo":
        return {"elbo": np.array([model._build_likelihood(X, Y, zs=zs)])}
    if entry == "elbo_grad":
        e = model._build_likelihood(X, Y, zs=zs, with_grad=True)
        eng.ctx.sync()
        return {"elbo": np.array([e]), "grad": eng.grad.cpu().numpy().copy()}
    if entry == "train_step":
        return _state_of(eng, model.train_step(0.01, X=X, Y=Y, zs=zs, sync=True))
    if X is None:                                            # train_step_minibatch: gather + ELBO + gradient + Adam in one call
        assert zs is None
        return _state_of(eng, model.train_step(0.01, sync=True))
    return _state_of(eng, model.train_step(0.01, X=X, Y=Y, zs=zs, sync=True))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("entry,shape", [(e, s) for e in TRAIN_ENTRIES for s in SHAPES
                                         if not (e == "train_step_minibatch" and s == "mixed")])   # (the one-call step takes no zs)
def test_device_draws_replay_bitwise(ctx, monkeypatch, entry, shape, mode):
    from doubly_stochastic_dgp.dgp import Minibatch
    _set_mode(monkeypatch, mode)
    mb = entry == "train_step_minibatch"
    X, Y, spec, state, A, S, num_data = _case(shape, minibatch_size=(240 if shape == "big" else 31) if mb else None)
    *_, B, _, _ = _case(shape, minibatch_size=A.minibatch_size)
    L = len(A.layers)
    if mb:
        Xa = Ya = None
        idx = Minibatch(X.shape[0], A.minibatch_size, seed=0).next_indices()      # the rows A's first step gathers
        Xb, Yb = X[idx], Y[idx]
    else:
        Xa, Ya, Xb, Yb = X, Y, X, Y
    n = Xb.shape[0]
    fixed = _fixed_zs(shape, A, S, n)
    A.engine(), B.engine()                                   # (device models created outside the counted calls)

    c0 = _launches(ctx)
    got = _call(entry, A, Xa, Ya, fixed)
    c1 = _launches(ctx)
    seed = A._seed
    sampled = [l for l in range(L - 1) if fixed is None or fixed[l] is None]      # the ELBO draws for the inner layers only
    zs = _replay_zs(ctx, A, seed, S, n, fixed, sampled)
    c2 = _launches(ctx)
    want = _call(entry, B, Xb, Yb, zs)
    c3 = _launches(ctx)

    _assert_bitwise(got, want, f"{entry} / {shape} / {mode}")
    # the draw path, as the launch counter sees it (the one-call minibatch step also differs by its gather launch: not counted)
    path = mode if (mode != "head" or _head_eligible(A)) else "side"
    if not mb:
        extra = (c1 - c0) - (c3 - c2)
        assert extra == (0 if path == "head" else len(sampled)), (path, extra, len(sampled))

    if mode == "head":                                       # once per entry and shape: the explicit draws through the oracle
        ref = OM.elbo(spec, state, Xb, Yb, _oracle_zs(zs), S, num_data=num_data)
        assert_allclose(want["elbo"][0], ref, rtol=1e-9)
        if entry == "elbo_grad":
            _, gref = OM.elbo_and_grad(spec, state, Xb, Yb, _oracle_zs(zs), S, num_data=num_data)
            g = B.engine().gradient_dict()
            for k in gref:
                err = np.max(np.abs(-gref[k] - g[k])) / (np.max(np.abs(gref[k])) + 1e-12)
                assert err <= 1e-7, (k, err)


# ---------------------------------------------------------------- 2. prediction entries (always in-line draws) and Engine.randn
PREDICT_ENTRIES = ["predict_all_layers", "predict_f", "predict_all_layers_full_cov", "sample_from_conditional"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("entry", PREDICT_ENTRIES)
def test_prediction_draws_replay_bitwise(ctx, monkeypatch, entry, shape):
    _set_mode(monkeypatch, "head")
    X, Y, spec, state, A, S, _ = _case(shape)
    *_, B, _, _ = _case(shape)
    L = len(A.layers)
    Xs = X[:9] if entry in ("predict_all_layers_full_cov", "sample_from_conditional") else X[:29]
    ns = Xs.shape[0]
    eA = A.engine()
    B.engine()
    fixed = _fixed_zs(shape, A, S, ns)

    if entry in ("predict_all_layers", "predict_f"):
        c0 = _launches(ctx)
        if entry == "predict_all_layers":
            got = A.propagate(Xs, S=S, zs=fixed)             # = predict_all_layers(Xs, S) when nothing is fixed
        else:
            got = A._build_predict(Xs, S=S, zs=fixed)        # = predict_f(Xs, S) when nothing is fixed
        c1 = _launches(ctx)
        sampled = [l for l in range(L) if fixed is None or fixed[l] is None]      # every layer, the last one included
        zs = _replay_zs(ctx, A, A._seed, S, ns, fixed, sampled)
        c2 = _launches(ctx)
        want = B.propagate(Xs, S=S, zs=zs) if entry == "predict_all_layers" else B._build_predict(Xs, S=S, zs=zs)
        c3 = _launches(ctx)
        assert (c1 - c0) - (c3 - c2) == len(sampled)         # in-line: one k_randn per sampled layer
        Fs_o, Fm_o, Fv_o = OM.propagate(spec, state, Xs, zs, S)
        if entry == "predict_all_layers":
            for l in range(L):
                for a, b, o in zip(got, want, (Fs_o, Fm_o, Fv_o)):
                    assert np.array_equal(a[l], b[l]), (entry, shape, l)
                    assert_allclose(b[l], o[l], rtol=1e-9, atol=1e-10)
        else:
            for a, b, o in zip(got, want, (Fm_o[-1], Fv_o[-1])):
                assert np.array_equal(a, b), (entry, shape)
                assert_allclose(b, o, rtol=1e-9, atol=1e-10)
        return

    # Engine.randn: seed 0x5eed, stream 2^32 | k for the engine's k-th draw
    k0 = getattr(eA, "_rng_calls", 0)
    if entry == "predict_all_layers_full_cov":
        got = A.propagate(Xs, full_cov=True, S=S, zs=fixed)      # = predict_all_layers_full_cov(Xs, S) when nothing is fixed
        assert eA._rng_calls == k0 + sum(1 for l in range(L) if fixed is None or fixed[l] is None)
        zs, k = [], k0
        for l, layer in enumerate(A.layers):
            if fixed is not None and fixed[l] is not None:
                zs.append(fixed[l])
            else:
                k += 1
                zs.append(_draw(ctx, ENGINE_SEED, 1 << 32 | k, (S, ns, layer.num_outputs)))
        want = B.propagate(Xs, full_cov=True, S=S, zs=zs)
        o = OM.propagate(spec, state, Xs, zs, S, full_cov=True)
        for l in range(L):
            for a, b, r in zip(got, want, o):
                assert np.array_equal(a[l], b[l]), (entry, shape, l)
                assert_allclose(b[l], r[l], rtol=1e-8, atol=1e-9)
        return

    F = np.tile(Xs[None], [S, 1, 1])
    for l in range(L):
        got = A.layers[l].sample_from_conditional(F, z=None)
        assert eA._rng_calls == k0 + l + 1
        z = _draw(ctx, ENGINE_SEED, 1 << 32 | (k0 + l + 1), (S, ns, A.layers[l].num_outputs))
        want = B.layers[l].sample_from_conditional(F, z=z)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (entry, shape, l)
        F = want[0]


# ---------------------------------------------------------------- 3. consecutive device-drawn steps
@pytest.mark.parametrize("mode", list(MODES))
def test_consecutive_minibatch_steps_replay_bitwise(ctx, monkeypatch, mode):
    """K = 8 asynchronous minibatch steps at n S Mp = 800 * 14 * 96 >= 2^18 (the two-stream schedule of tests/test_gpu_round3.py's
    _train_state) equal, after EVERY step, their replay from the same start with explicit draws of seeds 1 .. 8"""
    from doubly_stochastic_dgp.dgp import Minibatch
    _set_mode(monkeypatch, mode)
    K, N, D, M, S, BS = 8, 1000, 5, 96, 14, 800

    def build():
        rng = np.random.RandomState(5)
        X, Y = rng.randn(N, D), rng.randn(N, 2)
        Z = X[:M] + 0.05 * rng.randn(M, D)
        specs = [kern_spec("rbf", D, 1.1, 0.9), kern_spec("matern52", D, 0.8, 1.2), kern_spec("rbf", D, 0.9, 1.0)]
        _, _, model = make_case(X, Y, Z, specs, S=S, num_data=N, q_sqrt_scale=1e-2, minibatch_size=BS)
        return X, Y, model

    X, Y, A = build()
    eA = A.engine()
    snaps = []
    for _ in range(K):
        A.train_step(0.01)                                   # no synchronisation between the steps
        with ctx.torch.cuda.stream(ctx.tstream):
            snaps.append(eA.theta.clone())
    got_end = _state_of(eA)
    assert A._seed == K
    got = [s.cpu().numpy() for s in snaps]

    _, _, B = build()
    eB = B.engine()
    mb = Minibatch(N, BS, seed=0)
    blocks = {}
    for t in range(1, K + 1):
        idx = mb.next_indices()
        zs = [_draw(ctx, t, l, (S, BS, B.layers[l].num_outputs)) if l < 2 else None for l in range(3)]
        for l in range(2):
            blocks[(l, t)] = zs[l]
        B.train_step(0.01, X=X[idx], Y=Y[idx], zs=zs)
        eB.ctx.sync()
        th = eB.theta.cpu().numpy()
        assert np.all(np.isfinite(th))
        if not np.array_equal(got[t - 1], th):
            raise AssertionError(f"{mode}: parameters after step {t} differ from the replay with explicit draws "
                                 f"({int(np.count_nonzero(got[t - 1] != th))} of {th.size} entries)")
    _assert_bitwise(got_end, _state_of(eB), f"consecutive steps / {mode}")

    # 4. no reuse: no two (layer, step) blocks are equal, nor share their first 64 values
    keys = sorted(blocks)
    heads = {}
    for key in keys:
        h = blocks[key].ravel()[:64].tobytes()
        assert h not in heads, (key, heads.get(h))
        heads[h] = key
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(blocks[a], blocks[b]), (a, b)
