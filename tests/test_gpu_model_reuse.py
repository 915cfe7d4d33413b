"""A reused device model gives a fresh model's bits.

P1, history independence: a call (kind, n, S, inputs) made on a device model after any sequence of earlier calls returns the bits of the
same call made first on a fresh model with the same parameters and the same extents (n_max, s_max) — the workspace layout and alg_g are
fixed from the extents, so the fresh model is created at them.  Every reduction on the path has a fixed order and there are no
floating-point atomics, so no tolerance applies: float64 results are compared as uint64.

P2, read-only calls do not affect training: two models take the same optimiser steps, one of them also makes calls of other shapes and
kinds between the steps; theta, the Adam moments and every step's result scalars agree bit for bit.

tests/model_reuse_plan.py holds the sequences (one per model configuration, with the table of the schedule switches each shape flips),
the two data pools and the comparison.  P1 alone would hold if a used and a fresh model were wrong in the same way: for A, B and C one
small-shape gradient call of the used model is also checked against the oracle, at the tolerances of test_gpu_parity.py::_grad_check.

What a failure looks like: without ensure_plan's reset of part_big (tried while writing this file), A fails at its calls 3, 8, 9 and 13
and E at 5, 8 and 12 — every gradient call whose split-K plan has more diagonal slots than the previous plan filled — with tens of
thousands of gradient entries off by O(1) to O(1e4).  A call costs about a millisecond and a fresh model about ten, so a case runs in
well under a second.
"""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_allclose

from doubly_stochastic_dgp import _lib
from oracle import model as OM
from tests import model_reuse_plan as plan
from tests.helpers import kern_spec, make_case

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- model factories: the same parameters on every call
def _factory(name, white=False):
    cfg = plan.CONFIGS[name]
    n_max, s_max = cfg.extents
    D = cfg.widths[0]
    rng = np.random.RandomState(500 + ord(name))
    K = None
    if name == "F":
        K = cfg.DY
        X0 = 0.5 * rng.randn(n_max, D)
        Y0 = rng.choice(np.arange(K, dtype=np.float64), n_max).reshape(n_max, 1)
    else:
        X0, Y0 = rng.randn(n_max, D), rng.randn(n_max, cfg.DY)
    Z = X0[rng.permutation(n_max)[:cfg.M]] + 0.05 * rng.randn(cfg.M, D)
    if name == "A":
        specs = [kern_spec("rbf", 8, 1.0, 2.0)] * 3
    elif name == "B":
        specs = [kern_spec("matern52", 5, 1.1, 1.4, white_variance=0.03), kern_spec("rbf", 3, 0.9, 0.8 + rng.rand(3), True),
                 kern_spec("rbf", 3, 1.2, 0.7 + rng.rand(3), True)]
    elif name == "C":
        white = True
        specs = [kern_spec("rbf", 3, 1.1, 0.9, white_variance=0.03), kern_spec("matern52", 3, 0.8, 1.2)]
    elif name == "D":
        specs = [kern_spec("rbf", 4, 1.1, 0.9), kern_spec("matern52", 4, 0.8, 1.2)]
    elif name == "E":
        specs = [kern_spec("rbf", 6, 1.0, 1.5), kern_spec("matern52", 6, 0.9, 1.6)]
    else:
        specs = [kern_spec("rbf", 70, 1.0, 4.0), kern_spec("matern52", 5, 1.0, 0.8)]
    num_data = 5 * n_max

    def build():
        spec, state, model = make_case(X0, Y0, Z, specs, white=white, S=s_max, num_data=num_data, seed=7, num_classes=K)
        eng = model.engine()
        eng._ensure(n_max, s_max)
        assert (eng.n_max, eng.s_max) == (n_max, s_max)
        return spec, state, model

    return cfg, build, num_data, K


def _release(model):
    """free a fresh model's device side now (engine and layers refer to each other: the collector would get to it much later)"""
    eng = model.engine()
    eng.ctx.sync()
    eng._destroy()
    eng.workspace = None


# ---------------------------------------------------------------- one call and what it returns
def _host(t):
    return t.cpu().numpy().copy()


def _run_call(model, kind, n, S, pools, position):
    """the call of plan.py's table on `model`; returns {name: float64 array}.  Every draw is explicit or under an explicit seed, and the
    model's own seed counter is put back: nothing here moves model._draw_seed()."""
    from doubly_stochastic_dgp.distributed import shard_terms
    eng = model.engine()
    seed0, S0 = model._seed, model.num_samples
    model.num_samples = S
    try:
        if kind in ("C", "Cw"):
            out = {}
            for l, (layer, Xl) in enumerate(zip(model.layers, plan.conditional_inputs(pools, position, n))):
                if kind == "C":
                    mean, var = layer.conditional_ND(Xl)
                else:       # straight through the C-ABI: Engine.layer_conditional would re-create the model at the larger extent
                    assert n > eng.n_max * eng.s_max
                    eng._prepare_checked()
                    dX, dm, dv = eng.ctx.to_device(Xl), eng.ctx.empty(n, layer.num_outputs), eng.ctx.empty(n, layer.num_outputs)
                    _lib.check(eng.lib.dsdgp_model_layer_conditional(eng.model, l, C.c_void_p(dX.data_ptr()), n, C.c_void_p(dm.data_ptr()),
                                                                     C.c_void_p(dv.data_ptr())))
                    eng.ctx.sync()
                    mean, var = _host(dm), _host(dv)
                out[f"mean{l}"], out[f"var{l}"] = mean, var
            return out
        X, Y, zs = plan.call_inputs(pools, position, n, S)
        if kind in ("G", "Q", "Gd"):
            if kind == "Gd":
                scale, klw = shard_terms(model.num_data, n, 1)
                elbo = eng.elbo(X, Y, S, zs=None, seed=4242 + position, data_scale=scale, kl_weight=klw, with_grad=True)[0]
            else:
                q = kind == "Q"
                elbo = model._build_likelihood(X, Y, zs=zs, with_grad=True, grad_from_layer=1 if q else 0, grad_q_only=q)
            eng.ctx.sync()
            buf = _host(eng.gradbuf)
            if kind != "Q":
                return {"elbo": np.array([elbo]), "gradbuf": buf}
            # the other gradient entries are undefined after a (q_mu, q_sqrt)-only pass
            out = {"elbo": np.array([elbo]), "out4": buf[eng.n_theta:]}
            for l, layer in enumerate(model.layers[1:], 1):
                for p, off, cnt, _ in eng.entries:
                    if p is layer.q_mu or p is layer.q_sqrt:
                        out[f"l{l}.{'q_mu' if p is layer.q_mu else 'q_sqrt'}"] = buf[off:off + cnt]
            assert len(out) == 2 + 2 * (len(model.layers) - 1)
            return out
        if kind == "V":
            return {"elbo": np.array([model.compute_log_likelihood(X, Y, zs=zs)]), "E_log_p_Y": np.asarray(model.E_log_p_Y(X, Y, zs=zs))}
        if kind == "P":
            Fs, Fm, Fv = model.propagate(X, S=S, zs=zs)
            out = {}
            for l in range(len(model.layers)):
                out[f"F{l}"], out[f"mean{l}"], out[f"var{l}"] = Fs[l], Fm[l], Fv[l]
            return out
        assert kind == "E", kind
        res = model.evaluate(X, Y, S, batch_size=max(1, (2 * n + 2) // 3), zs=zs, return_rows=True)      # a ragged second batch
        out = {k: np.asarray(v, dtype=np.float64) for k, v in res.items() if k != "n"}
        D = model.layers[-1].num_outputs                                                                  # the accumulator itself
        acc, rows = eng.ctx.empty(3, D), eng.ctx.empty(n, D, 3)
        keep = eng.evaluate_batch(eng.ctx.to_device(X), eng.ctx.to_device(Y), S, acc, False, zs=zs, seed=0, rows=rows)
        eng.ctx.sync()
        del keep
        out["acc"], out["acc_rows"] = _host(acc), _host(rows)
        return out
    finally:
        model._seed, model.num_samples = seed0, S0


# ---------------------------------------------------------------- 1. the sequence driver
def _oracle_anchor(spec, state, model, got, X, Y, zs, S, num_data):
    ref, gref = OM.elbo_and_grad(spec, state, X, Y, zs, S, num_data=num_data)
    assert_allclose(got["elbo"][0], ref, rtol=1e-9)
    g = model.engine().gradient_dict()
    worst = {k: np.max(np.abs(-gref[k] - g[k])) / (np.max(np.abs(gref[k])) + 1e-12) for k in gref}
    bad = {k: v for k, v in worst.items() if not v <= 1e-7}
    assert not bad, f"gradient mismatch (rel to max entry): {bad}; all: {worst}"


def run_sequence(build, cfg, pools, num_data):
    """Runs cfg.seq on one used model; every call also first on a fresh model of the same extents; asserts P1 on everything a call
    returns (all calls are made before the first failure is reported: a later call tells which buffer an earlier one spoilt)."""
    spec, state, used = build()
    eng = used.engine()
    generation = eng.generation
    failures = []
    for i, (kind, n, S) in enumerate(cfg.seq):
        got = _run_call(used, kind, n, S, pools, i)
        if i == cfg.anchor:
            assert kind == "G" and n <= 100 and S <= 3
            _oracle_anchor(spec, state, used, got, *plan.call_inputs(pools, i, n, S), S, num_data)
        _, _, fresh = build()
        want = _run_call(fresh, kind, n, S, pools, i)
        _release(fresh)
        for k, v in want.items():
            assert np.all(np.isfinite(v)), (cfg.name, i, kind, k)
        try:
            plan.assert_same_bits(got, want, f"config {cfg.name}, call {i} {kind} {(n, S)} after {cfg.seq[i - 1] if i else 'creation'}")
        except AssertionError as e:
            failures.append(str(e))
    assert eng.generation == generation and (eng.n_max, eng.s_max) == cfg.extents       # nothing was re-created on the way
    _release(used)
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------- 2. one case per model configuration
CASES = [("A", False), ("B", False), ("C", True), ("D", False), ("D", True), ("E", False), ("F", False)]


@pytest.mark.parametrize("name,white", CASES, ids=[f"{n}{'-white' if w and n == 'D' else ''}" for n, w in CASES])
def test_reused_model_gives_a_fresh_models_bits(monkeypatch, name, white):
    monkeypatch.delenv("DSDGP_NO_OVERLAP", raising=False)
    if name == "D":
        monkeypatch.setenv("DSDGP_FORCE", "gemm_mp=16")
    else:
        monkeypatch.delenv("DSDGP_FORCE", raising=False)
    cfg, build, num_data, K = _factory(name, white)
    pools = {w: plan.make_pool(cfg, w, num_classes=K) for w in "ab"}
    run_sequence(build, cfg, pools, num_data)


# ---------------------------------------------------------------- 4. P2: read-only calls between optimiser steps
def _train(build, cfg, case, pools, with_reads):
    from doubly_stochastic_dgp.distributed import shard_terms
    _, _, model = build()
    eng = model.engine()
    generation = eng.generation
    n, S = case["step"]
    model.num_samples = S
    n_max = cfg.extents[0]
    Xall, Yall = eng.ctx.to_device(pools["a"]["X"][:n_max]), eng.ctx.to_device(pools["a"]["Y"][:n_max])
    idx = eng.ctx.torch.as_tensor(np.random.RandomState(5).permutation(n_max).astype(np.int64)).to(Xall.device)
    out = {}
    for k in range(plan.P2_STEPS):
        if k in plan.P2_MINIBATCH_STEPS:
            scale, klw = shard_terms(model.num_data, n, 1)
            eng.train_step_minibatch(Xall, Yall, idx, k * n, n, S, seed=900 + k, data_scale=scale, kl_weight=klw, lr=0.01)
        else:
            X, Y, zs = plan.call_inputs(pools, 2 * k + 1, n, S)           # odd positions: pool a
            seed0 = model._seed
            model.train_step(0.01, X=X, Y=Y, zs=zs)
            model._seed = seed0
        eng.ctx.sync()
        out[f"out4[{k}]"] = _host(eng.out4)
        assert out[f"out4[{k}]"][3] == 0.0
        if with_reads and k < len(case["between"]):
            for j, (kind, nn, SS) in enumerate(case["between"][k]):
                _run_call(model, kind, nn, SS, pools, 2 * (k + j))         # even positions: pool b; results are not the point here
    eng.ctx.sync()
    out.update(theta=_host(eng.theta), adam_m=_host(eng.adam_m), adam_v=_host(eng.adam_v), adam_t=np.array([float(eng.adam_t)]))
    assert eng.generation == generation
    _release(model)
    return out


@pytest.mark.parametrize("name", list(plan.P2_CASES))
def test_read_only_calls_between_steps_leave_training_unchanged(monkeypatch, name):
    monkeypatch.delenv("DSDGP_NO_OVERLAP", raising=False)
    monkeypatch.delenv("DSDGP_FORCE", raising=False)
    cfg, build, _, K = _factory(name)
    case = plan.P2_CASES[name]
    pools = {w: plan.make_pool(cfg, w, num_classes=K) for w in "ab"}
    plain = _train(build, cfg, case, pools, with_reads=False)
    busy = _train(build, cfg, case, pools, with_reads=True)
    assert plain["adam_t"][0] == plan.P2_STEPS
    assert np.any(plain["theta"] != _train_start_theta(build))                # the steps did move the parameters
    plan.assert_same_bits(busy, plain, f"config {name}: training with read-only calls in between against training alone")


def _train_start_theta(build):
    _, _, model = build()
    eng = model.engine()
    eng._upload_if_needed()
    eng.ctx.sync()
    th = _host(eng.theta)
    _release(model)
    return th
