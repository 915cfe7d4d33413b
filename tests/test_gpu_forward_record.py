"""-m gpu: the lifetime of what a forward pass leaves for the reverse pass (csrc/forward_plan.hpp: FwdRecord — each layer's input, draws,
row counts and whether c_d was kept, the step's extents, who wrote the last layer's adjoints, the pending fused last launch).

One device model makes, in this order: a gradient at (n, S) with the caller's draws; a propagate at a smaller (n', S') with draws from a
seed; a value at (n, S); a saved forward pass at (n', S') from a seed and its reverse pass from the caller's adjoints; the gradient at
(n, S) again.  Every result is compared bit for bit (float64 as uint64) with the same call made FIRST on a fresh model with the same
parameters, created at the same extents — so nothing a reverse pass reads may be left over from an earlier forward pass of another shape
or kind.  And a reverse pass from adjoints is refused (DSDGP_ERR_BAD_ARG, nothing written) once a propagate came between it and its
saved forward pass.

Two models: L = 3, M = 20, D = 3 at n = 40, S = 3 — the head launch draws for the inner layers, the last layer runs as its two chains;
L = 2, M = 128, D = 5 at n = 200, S = 2 — the last layer of a gradient runs as the fused launch (layer_last.hip), which the record holds
pending between the two passes.  At these extents the fused launch needs the algebraic dl/dKu assembly forced on (DSDGP_FORCE alg_g=1:
the heuristic asks for S n >= 4 Mp rows); that the two models do take the head launch / the fused launch is checked by launch counts
against a model with that launch forced off."""
import ctypes as C

import numpy as np
import pytest

from doubly_stochastic_dgp import _lib
from tests.helpers import kern_spec, make_case

pytestmark = pytest.mark.gpu

#                 L   M   D   n   S   smaller (n', S')  DSDGP_FORCE  the launch under test, forced off
MODELS = {
    "head": (3, 20, 3, 40, 3, (25, 2), None, "head=0"),
    "fused_last": (2, 128, 5, 200, 2, (70, 1), "alg_g=1", "alg_g=1,last_fuse=0"),
}
ERR_BAD_ARG = -1


def _factory(name):
    L, M, D, n, S, small, _, _ = MODELS[name]
    rng = np.random.RandomState(900 + len(name))
    X, Y = rng.randn(n, D), rng.randn(n, 1)
    Z = X[rng.permutation(n)[:M]] + 0.05 * rng.randn(M, D) if M <= n else rng.uniform(-2.0, 2.0, (M, D))
    specs = [kern_spec("rbf" if l % 2 == 0 else "matern52", D, 1.0 + 0.1 * l, 1.2) for l in range(L)]
    outs = [D] * (L - 1) + [1]
    n2, S2 = small
    data = dict(X=X, Y=Y, zs=[rng.randn(S, n, d) for d in outs], X2=X[:n2].copy(), S2=S2, dm=rng.randn(S2, n2, 1), dv=rng.randn(S2, n2, 1))

    def build():
        _, _, model = make_case(X, Y, Z, specs, S=S, num_data=5 * n, seed=9)
        eng = model.engine()
        eng._ensure(n, S)
        assert (eng.n_max, eng.s_max) == (n, S)
        return model

    return build, data, S


def _release(model):
    eng = model.engine()
    eng.ctx.sync()
    eng._destroy()
    eng.workspace = None


def _host(t):
    return t.cpu().numpy().copy()


def _call(eng, kind, d, S):
    """one call of the sequence -> {name: float64 array}"""
    if kind in ("G", "V"):
        out = {"out4": np.array(eng.elbo(d["X"], d["Y"], S, zs=d["zs"], data_scale=5.0, with_grad=kind == "G"))}
        if kind == "G":
            out["grad"] = _host(eng.gradbuf)
        return out
    if kind == "P":
        Fs, means, vs = eng.propagate(d["X2"], d["S2"], seed=77)
        eng.ctx.sync()
        return {f"{k}{l}": _host(t) for k, ts in (("F", Fs), ("mean", means), ("var", vs)) for l, t in enumerate(ts)}
    mean, var = eng.forward_saved(d["X2"], d["S2"], seed=78)
    out4 = eng.backward_adjoints(d["dm"], d["dv"])
    return {"mean": _host(mean), "var": _host(var), "out4": np.array(out4), "grad": _host(eng.gradbuf)}


def _differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not (a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)))]


@pytest.mark.parametrize("name", list(MODELS))
def test_every_call_of_a_used_model_gives_a_fresh_models_bits(name, monkeypatch):
    force, off = MODELS[name][6], MODELS[name][7]
    build, d, S = _factory(name)
    count = _lib.load().dsdgp_launch_count
    # the model takes the launch it is here for: with it forced off the same gradient call takes one launch more
    launches = {}
    for setting in (off, force):
        if setting:
            monkeypatch.setenv("DSDGP_FORCE", setting)
        else:
            monkeypatch.delenv("DSDGP_FORCE", raising=False)
        probe = build()
        n0 = count()
        _call(probe.engine(), "G", d, S)
        launches[setting] = count() - n0
        _release(probe)
    print(name, "launches of the gradient call:", launches)
    assert launches[off] == launches[force] + 1
    used = build()
    sequence = ("G", "P", "V", "SB", "G")
    for i, kind in enumerate(sequence):
        got = _call(used.engine(), kind, d, S)
        fresh = build()
        want = _call(fresh.engine(), kind, d, S)
        _release(fresh)
        bad = _differing(got, want)
        assert not bad, f"{name}: call {i} ({kind}) of the used model differs from a fresh model's in {bad}"
        assert all(np.isfinite(v).all() for v in want.values())
    _release(used)


@pytest.mark.parametrize("name", list(MODELS))
def test_a_propagate_between_the_saved_pass_and_its_reverse_pass_is_refused(name, monkeypatch):
    if MODELS[name][6]:
        monkeypatch.setenv("DSDGP_FORCE", MODELS[name][6])
    build, d, S = _factory(name)
    model = build()
    eng = model.engine()
    _call(eng, "G", d, S)
    before = _host(eng.gradbuf).view(np.uint64)
    eng.forward_saved(d["X2"], d["S2"], seed=78)
    eng.propagate(d["X2"], d["S2"], seed=77)
    dm, dv = eng.ctx.to_device(d["dm"]), eng.ctx.to_device(d["dv"])
    # straight through the C-ABI: the refusal under test is the library's, whatever the wrapper keeps track of itself
    rc = eng.lib.dsdgp_model_backward_adjoints(eng.model, C.c_void_p(dm.data_ptr()), C.c_void_p(dv.data_ptr()), C.c_double(1.0),
                                              C.c_void_p(eng.out4.data_ptr()))
    assert rc == ERR_BAD_ARG
    assert "forward_saved" in eng.lib.dsdgp_last_error().decode()
    eng.ctx.sync()
    assert np.array_equal(before, _host(eng.gradbuf).view(np.uint64))
    # ... and the pair made again stands
    got = _call(eng, "SB", d, S)
    fresh = build()
    bad = _differing(got, _call(fresh.engine(), "SB", d, S))
    _release(fresh)
    _release(model)
    assert not bad
