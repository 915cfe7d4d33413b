"""-m gpu: every entry of theta, m and v after an Adam step against a long-double evaluation of the same step (tests/adam_reference.py),
on both ways into adam_sweep (csrc/model_kernels.hpp): the separate k_adam launch behind dsdgp_model_adam_step and the Adam blocks of
k_tail inside dsdgp_model_train_step.

(a) separate launch on injected state: every small layout x every hyper-parameter set of tests/adam_cases.py;
(b) three fused training steps per small layout, the reference taking the gradient the device left behind (white=True: the fallback);
(c) the large layout (n_theta = 5 251 075: all four slots of a thread's batch, two passes, a single-entry tail): one fused step, then
    one injected separate step; a second layout of that size with a (class 2, class 1) pair in the second pass: one fused step;
(d) a failed Ku factorisation leaves theta, m and v as they were, on both paths.
The asserted bar is twice the first-order bound B of a float64 evaluation; entries of mask class 0 must keep their bits.
DSDGP_ADAM_PROFILE=<file> writes the measured ratios (profiles/adam_direct_errors.md)."""
import os

import numpy as np
import pytest

from tests import adam_cases as AC
from tests import adam_reference as R

pytestmark = pytest.mark.gpu

_PROFILE = os.environ.get("DSDGP_ADAM_PROFILE")
_ROWS, _LARGE_ROWS = [], []
_DEFAULT = AC.PARAM_SETS["default_t1"]


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    if not _PROFILE or not _ROWS:
        return
    with open(_PROFILE, "w") as f:
        f.write("# Adam step, entry by entry: device against long double (tests/test_gpu_adam_direct.py)\n\n"
                "`ratio`: the largest `|device - long double| / B` over the live entries, `B` the first-order bound of a float64\n"
                "evaluation (tests/adam_reference.py): 1 is at the bound, 2 at the asserted bar.  `live`: entries of mask class 1 or 2,\n"
                "`dead`: class 0 (frozen, or above the diagonal of a q_sqrt), which kept their bits.  `separate`: the k_adam launch on\n"
                "injected state; `fused`: a training step (Adam inside k_tail), `fallback`: a training step of a white=True model\n"
                "(ELBO, then k_adam); the number behind either is the step t.\n\n"
                "| layout | path | hyper-parameters | ratio theta | ratio m | ratio v | live | dead |\n|---|---|---|---|---|---|---|---|\n")
        for row in _ROWS:
            f.write("| %s | %s | %s | %.3f | %.3f | %.3f | %d | %d |\n" % row)
        if _LARGE_ROWS:
            f.write("\n## Large layouts: live and dead entries and the largest ratios per slot of the four-pair batch and pass\n\n"
                    "(slot -1: the single entry behind the last pair of an odd n_theta)\n\n"
                    "| layout | path | slot | pass | live | dead | ratio theta | ratio m | ratio v |\n|---|---|---|---|---|---|---|---|---|\n")
            for row in _LARGE_ROWS:
                f.write("| %s | %s | %d | %d | %d | %d | %.3f | %.3f | %.3f |\n" % row)


# ------------------------------------------------------------------------------------------------ plumbing
def _get(eng, t):
    eng.ctx.sync()
    return t.cpu().numpy().copy()


def _put(eng, t, arr):
    t.copy_(eng.ctx.torch.as_tensor(np.ascontiguousarray(arr, dtype=np.float64)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _launches(eng):
    return int(eng.lib.dsdgp_launch_count())


def _engine_of(model, N, S):
    eng = model.engine()
    eng._ensure(N, S)
    eng._upload_if_needed()
    return eng


def _check(layout, path, pset, mask, before, g, after, h, by_slot=False):
    """before, after: (theta, m, v).  Dead entries keep their bits; live ones sit within BAR x B of the long-double step."""
    live = mask != 0
    n = mask.size
    for key, b, a in zip(("theta", "m", "v"), before, after):
        moved = np.flatnonzero(~live & (_bits(a) != _bits(b)))
        assert moved.size == 0, (layout, path, pset, key, "class-0 entries moved", moved[:8].tolist(), a[moved[:8]].tolist())
    ref = R.adam_ld(before[0], g, before[1], before[2], live, h["lr"], h["b1"], h["b2"], h["eps"], h["t"])
    worst, rs = {}, {}
    for key, a in zip(("theta", "m", "v"), after):
        r = R.ratios(a, ref[key], ref["B_" + key], live)
        rs[key] = r
        i = int(np.argmax(np.where(np.isnan(r), np.inf, r)))
        u, p = AC.slot_and_pass(i, n)
        worst[key] = (float(r[i]), i, int(u), int(p))
        print("%-20s %-10s %-15s %-5s device / B = %.3f (entry %d, slot %d, pass %d)" % ((layout, path, pset, key) + worst[key]))
    if _PROFILE:
        _ROWS.append((layout, path, pset, worst["theta"][0], worst["m"][0], worst["v"][0], int(live.sum()), int(n - live.sum())))
        if by_slot:
            u, p = AC.slot_and_pass(np.arange(n), n)
            for a, b in sorted(set(zip(u.tolist(), p.tolist()))):
                sel = (u == a) & (p == b)
                _LARGE_ROWS.append((layout, path, a, b, int((sel & live).sum()), int((sel & ~live).sum())) +
                                   tuple(float(rs[k][sel].max()) for k in ("theta", "m", "v")))
    for key in ("theta", "m", "v"):
        ratio, i, u, p = worst[key]
        assert ratio <= R.BAR, (layout, path, pset, key, "ratio %.4g at entry %d (class %d, slot %d, pass %d): device %r, long double %r"
                                % (ratio, i, int(mask[i]), u, p, float(after[("theta", "m", "v").index(key)][i]), float(ref[key][i])))
    return ref


def _injected_step(eng, mask, h, seed):
    """adam_step from the generator's state -> (before, g, after, zero, grad afterwards)"""
    th, g, m, v, zero = R.make_inputs(mask, seed, h["b1"])
    for t, a in ((eng.theta, th), (eng.grad, g), (eng.adam_m, m), (eng.adam_v, v)):
        _put(eng, t, a)
    eng.adam_t = h["t"] - 1
    n0 = _launches(eng)
    eng.adam_step(h["lr"], h["b1"], h["b2"], h["eps"])
    assert _launches(eng) - n0 == 1
    after = tuple(_get(eng, t) for t in (eng.theta, eng.adam_m, eng.adam_v))
    return (th, m, v), g, after, zero, _get(eng, eng.grad)


def _check_injected(layout, eng, mask, h, pset, seed, by_slot=False):
    before, g, after, zero, g_after = _injected_step(eng, mask, h, seed)
    assert _same_bits(g_after, g), "the step wrote to the gradient"
    _check(layout, "separate", pset, mask, before, g, after, h, by_slot=by_slot)
    assert zero.any() and _same_bits(after[0][zero], before[0][zero])                   # g = m = v = 0: theta as it was, moments +0
    for a in after[1:]:
        assert np.all(_bits(a[zero]) == 0)
    again = _injected_step(eng, mask, h, seed)[2]
    for a, b in zip(after, again):
        assert _same_bits(a, b), "a second run from the same state gave other bits"


# ------------------------------------------------------------------------------------------------ (a) separate launch, injected state
_SMALL_ENGINES = {}


def _small_engine(layout):
    if layout not in _SMALL_ENGINES:
        model, X, Y, zs, S = AC.build_small(layout)
        eng = _engine_of(model, X.shape[0], S)
        _SMALL_ENGINES[layout] = (model, eng, R.mask_from_model(model))
    return _SMALL_ENGINES[layout]


@pytest.mark.parametrize("pset", list(AC.PARAM_SETS))
@pytest.mark.parametrize("layout", list(AC.SMALL))
def test_separate_step_on_injected_state(layout, pset):
    model, eng, mask = _small_engine(layout)
    assert mask.size == eng.n_theta
    _check_injected(layout, eng, mask, AC.PARAM_SETS[pset], pset, seed=1000 + 17 * list(AC.PARAM_SETS).index(pset))


# ------------------------------------------------------------------------------------------------ (b) fused steps / the white=True fallback
def _poison_dead_moments(eng, mask):
    """distinct finite non-zero m and v on the class-0 entries (the device leaves zeros there otherwise, which hide a stray update)"""
    dead = np.flatnonzero(mask == 0)
    for t, a in ((eng.adam_m, -(2e5 + dead)), (eng.adam_v, 3e5 + dead)):
        x = _get(eng, t)
        x[dead] = a
        _put(eng, t, x)


def _train_step_checked(layout, path, eng, mask, X, Y, zs, S, t, data_scale, by_slot=False):
    """one eng.train_step at step t, checked against the long-double step on the gradient the device left -> its launch count"""
    before = tuple(_get(eng, x) for x in (eng.theta, eng.adam_m, eng.adam_v))
    assert eng.adam_t == t - 1
    h = dict(_DEFAULT, t=t)
    n0 = _launches(eng)
    eng.train_step(X, Y, S, zs=zs, seed=0, data_scale=data_scale, lr=h["lr"], beta1=h["b1"], beta2=h["b2"], eps=h["eps"])
    count = _launches(eng) - n0
    out4 = _get(eng, eng.out4)
    assert out4[3] == 0.0 and np.isfinite(out4[0])
    g = _get(eng, eng.grad)
    assert np.all(np.isfinite(g)) and np.any(g[mask != 0] != 0.0)
    after = tuple(_get(eng, x) for x in (eng.theta, eng.adam_m, eng.adam_v))
    _check(layout, "%s %d" % (path, t), "default", mask, before, g, after, h, by_slot=by_slot)
    return count


@pytest.mark.parametrize("layout", list(AC.SMALL))
def test_training_steps_against_the_device_gradient(layout):
    model, X, Y, zs, S = AC.build_small(layout)
    white = AC.SMALL[layout]["white"]
    eng = _engine_of(model, X.shape[0], S)
    mask = R.mask_from_model(model)
    _poison_dead_moments(eng, mask)
    scale = AC.NUM_DATA / X.shape[0]
    counts = [_train_step_checked(layout, "fallback" if white else "fused", eng, mask, X, Y, zs, S, t, scale) for t in (1, 2, 3)]
    # the path it claims to be: a fused step costs what the gradient evaluation alone costs, ELBO + separate step one launch more
    n0 = _launches(eng)
    eng.elbo(X, Y, S, zs=zs, seed=0, data_scale=scale, with_grad=True, sync=False)
    n_elbo = _launches(eng) - n0
    eng.adam_step()
    assert _launches(eng) - n0 == n_elbo + 1
    eng.ctx.sync()
    assert counts == [n_elbo + (1 if white else 0)] * 3, (counts, n_elbo)


# ------------------------------------------------------------------------------------------------ (c) large layout
@pytest.fixture(scope="module")
def large():
    model, X, Y, zs, S = AC.build_large()
    eng = _engine_of(model, X.shape[0], S)
    assert eng.n_theta == AC.LARGE_N_THETA
    return model, eng, R.mask_from_model(model), X, Y, zs, S


def test_large_layout_fused_step(large):
    model, eng, mask, X, Y, zs, S = large
    assert eng.adam_t == 0
    _poison_dead_moments(eng, mask)
    count = _train_step_checked("m1024_large", "fused", eng, mask, X, Y, zs, S, 1, 1000 / X.shape[0], by_slot=True)
    n1 = _launches(eng)
    eng.elbo(X, Y, S, zs=zs, seed=0, data_scale=1000 / X.shape[0], with_grad=True, sync=False)
    eng.ctx.sync()
    assert count == _launches(eng) - n1


def test_large_layout_separate_step_on_injected_state(large):
    model, eng, mask, X, Y, zs, S = large
    _check_injected("m1024_large", eng, mask, dict(_DEFAULT, t=2), "default_t2", seed=77, by_slot=True)


def test_large_mixed_layout_fused_step():
    """tests/adam_cases.py, large mixed layout: two class-2 entries (white variance, likelihood variance) share a pair with a class-1
    entry that the sweep reaches in its second pass, after the owner blocks' updates"""
    model, X, Y, zs, S = AC.build_large(mixed=True)
    eng = _engine_of(model, X.shape[0], S)
    mask = R.mask_from_model(model)
    assert eng.n_theta == AC.LARGE_MIXED_N_THETA
    for (a, b), classes in AC.LARGE_MIXED_PAIRS.items():
        assert (mask[a], mask[b]) == classes
    _poison_dead_moments(eng, mask)
    _train_step_checked("m1024_large_mixed", "fused", eng, mask, X, Y, zs, S, 1, 1000 / X.shape[0], by_slot=True)


# ------------------------------------------------------------------------------------------------ (d) failed factorisation
def test_failed_factorisation_leaves_parameters_and_moments_untouched():
    """csrc/model_kernels.hpp, chol_failed: a reported non-positive pivot of Ku (duplicated inducing points, jitter -1e-3 — the
    construction of test_gpu_parity.py::test_cholesky_failure_raises) skips the update in k_tail and in k_adam"""
    from doubly_stochastic_dgp import _lib, settings
    from tests.helpers import kern_spec, make_case
    rng = np.random.RandomState(0)
    X = rng.randn(30, 2)
    Z = np.concatenate([X[:10], X[:10]])
    with settings.temp_jitter(1e-6):
        _, _, model = make_case(X, rng.randn(30, 1), Z, [kern_spec("rbf", 2)], S=1, randomize=False)
        eng = model.engine()
        model.train_step(0.01, sync=True)                                   # a good step: m and v are non-zero from here on
    state = (eng.theta, eng.adam_m, eng.adam_v)
    with settings.temp_jitter(-1e-3):
        eng._ensure(30, 1)
        eng._upload_if_needed()                                             # the jitter change re-creates the device model and uploads theta
        snap = tuple(_get(eng, t) for t in state)
        assert all(np.any(a != 0.0) for a in snap[1:])
        model.train_step(0.01)                                              # asynchronous: reported by the next synchronising call
        with pytest.raises(_lib.CholeskyError):
            model.train_step(0.01, sync=True)
        for key, t, a in zip(("theta", "m", "v"), state, snap):
            assert _same_bits(_get(eng, t), a), "fused step after a failed factorisation moved " + key
        _put(eng, eng.grad, 1.0 + 0.25 * np.arange(eng.n_theta))
        eng.adam_step(0.01)
        for key, t, a in zip(("theta", "m", "v"), state, snap):
            assert _same_bits(_get(eng, t), a), "separate step after a failed factorisation moved " + key
    with settings.temp_jitter(1e-6):                                        # the model is still usable: the next good step moves theta again
        eng._ensure(30, 1)
        eng._upload_if_needed()
        th0 = _get(eng, eng.theta)
        model.train_step(0.01, sync=True)
        th1 = _get(eng, eng.theta)
        live = R.mask_from_model(model) != 0
        assert np.all(np.isfinite(th1)) and np.count_nonzero(th1[live] != th0[live]) >= 0.9 * live.sum() and _same_bits(th1[~live], th0[~live])
