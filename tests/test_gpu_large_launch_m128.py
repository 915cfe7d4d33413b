"""The large-launch chain instances at a padded inducing count of 128, against the oracle.

At Mp = 128 the chain kernels pick their instance by the number of 16-row blocks of a launch (csrc/chain_policy.hpp: sm_small / sm_nw):
the forward chain takes the 8-wave instance up to 160 row blocks and the 4-wave one (early-mean form) beyond, the backward chain the
8-wave instance up to 768 row blocks and the 4-wave one (paired d-loop) beyond.  Every other M = 128 test of the suite stays on the
8-wave side except the two full-size config-2 tests, which cover one point of the 4-wave side (RBF, white = False, D_out 8 and 1,
Gaussian, 1250 full row blocks, fused last layer).  The cases here sit one ragged row block past each threshold — 4 x 3073 = 12 292
rows = 769 blocks with 4 live rows in the last one for the training pass, 4 x 641 = 2 564 rows = 161 blocks for the forward-only
calls — and each asserts that arithmetic, so a change of shape cannot drop it back onto the 8-wave instance unnoticed.  They run the
4-wave instances as Matern-5/2, whitened, with the likelihood epilogue (LIK), with kept c_d (CS), with padded inducing rows
(120 -> 128), behind k_adj_prep, with the adjoint prologue (up_dF) on a first layer of 769 blocks, and with D_out = 9 (epilogue
groups 8 + 1).  Bars are the suite's own: ELBO rtol 1e-9, every gradient block 1e-7 of its largest entry (test_gpu_parity._grad_check),
per-layer F / mean / var rtol 1e-9 atol 1e-10.  The oracle runs live, about half a second per evaluation at these shapes.

What a failure looks like: with one accumulator of the paired Ku^-1 / Lu^-T product (bb[0] behind chain_dense2 / chain_range2) scaled by
1 + 1e-3 under `if constexpr (NW == 4 && MPB == 8)` — a change that only the 4-wave Mp = 128 backward instance sees, tried once while
writing this file — eight of the ten training cases fail: (a), (b), (c), (e), (g), (d) with `last_fuse=0` and both forms of (f), with
the Z, q_mu, q_sqrt and kernel hyper-parameter gradients of the layer below the mutated launch and the Z and kernel hyper-parameter
gradients of its own layer off by 3e-4 .. 1e-2 of their largest entry ((f), whose first layer is the mutated launch: up to 7e-2),
while the ELBO and the layer's own q_mu / q_sqrt gradients stay at 1e-14.  (h) passes, as it must — the CS instance does not take the
paired form — and so does (d) in its default form, whose last layer is the fused launch and whose first layer has 193 blocks.  Of the
149 tests of test_gpu_parity.py and test_gpu_round6.py the same change fails one, test_full_size_cfg2_against_oracle (l0.Z at 8e-5
against its 1e-5 bar); every other test there stays green.  Unmutated, the worst gradient block of any case is 2e-12, the ELBOs sit at
4e-14 or better, and the two instances of the conditional agree to 8e-16 absolute.
"""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import dgp_oracle as O
from oracle import model as OM
from tests.helpers import kern_spec, make_case
from tests.test_gpu_parity import _grad_check

pytestmark = pytest.mark.gpu

FWD_8W_BLOCKS = 160      # chain_policy.hpp: SM_SMALL_BLOCKS
BWD_8W_BLOCKS = 768      # chain_policy.hpp: SM_BWD_RESIDENT_8W
N_BWD, N_FWD, S4 = 3073, 641, 4


def _blocks(rows):
    return -(-rows // 16)


def _set_force(monkeypatch, force):
    """DSDGP_FORCE is read when the device model is created: set (or clear) it before make_case"""
    if force:
        monkeypatch.setenv("DSDGP_FORCE", force)
    else:
        monkeypatch.delenv("DSDGP_FORCE", raising=False)


def _build(specs, N, DY, M=128, S=S4, white=False, num_classes=None, seed=0):
    """randn inputs, Z a permuted subset of X plus 0.02 randn, num_data = 4 N, explicit zs, jitter 1e-6.  The lengthscales of the cases
    are short enough for their input dimension that cond(Ku + jitter) stays near 1e3 .. 1e5 (an RBF at lengthscale 1.2 on 128 of these
    points in three dimensions reaches 5e7): the oracle's own rounding, eps x cond, stays orders of magnitude below the bars."""
    rng = np.random.RandomState(seed)
    D = specs[0]["input_dim"]
    X = rng.randn(N, D)
    if num_classes:
        Y = rng.randint(0, num_classes, size=(N, 1)).astype(np.float64)
        DY = num_classes
    else:
        Y = rng.randn(N, DY)
    Z = X[rng.permutation(N)[:M]] + 0.02 * rng.randn(M, D)
    spec, state, model = make_case(X, Y, Z, specs, white=white, jitter=1e-6, S=S, num_data=4 * N, seed=seed + 1, num_classes=num_classes)
    zs = [rng.randn(S, N, s["input_dim"]) for s in specs[1:]] + [rng.randn(S, N, DY)]
    return X, Y, spec, state, model, zs


def _grads(model):
    return {k: np.asarray(v).copy() for k, v in model.engine().gradient_dict().items()}


# ---------------------------------------------------------------- 1. training pass
def _case_a(rng):
    return dict(specs=[kern_spec("matern52", 4, 1.1, 0.8 + rng.rand(4), True, white_variance=0.02),
                       kern_spec("matern52", 4, 0.9, 0.9 + rng.rand(4), True, white_variance=0.02)], DY=3)


TRAIN = {
    # Matern instances in both directions; D_Y = 3 Gaussian: the LIK forward instance on the last layer
    "a-matern52-ard": dict(make=_case_a, twice=True),
    # WHITE instances in both directions, chain_range2 in the backward Lu^-T product, dl/dKu through E A^T (split-K) at scale
    "b-rbf-white": dict(specs=[kern_spec("rbf", 5, 1.1, 1.2)] * 2, DY=2, white=True, twice=True),
    # padded inducing rows (120 -> 128) in the 4-wave instances
    "c-matern52-white-M120": dict(specs=[kern_spec("matern52", 4, 1.1, 1.2)] * 2, DY=1, white=True, M=120),
    # D_out = 9: epilogue groups 8 + 1 in the 4-wave forward instance, nine outputs in the paired d-loop
    "e-rbf-three-layers-D9": dict(specs=[kern_spec("rbf", 9, 1.1, 1.8)] * 3, DY=1),
    # k_adj_prep (non-Gaussian likelihood) feeding the 4-wave backward chain
    "g-rbf-multiclass3": dict(specs=[kern_spec("rbf", 4, 1.1, 0.9)] * 2, DY=None, num_classes=3),
    # the CS = true 4-wave backward instance (c_d kept by the forward chain)
    "h-rbf-csave": dict(specs=[kern_spec("rbf", 4, 1.1, 0.9)] * 2, DY=3, force="save_c=2,cs_min_blocks=0,cs_min_dout=1"),
}


@pytest.mark.parametrize("name", list(TRAIN))
def test_training_pass_against_the_oracle(monkeypatch, name):
    """ELBO and every gradient block of a two-layer (e: three-layer) model whose inner launches have S N = 4 x 3073 = 12 292 rows:
    Rin = 12 292 -> ldA = 12 304 = 769 row blocks > 768 (backward chain: 4-wave), and > 160 (forward chain: 4-wave; the first layer's
    Rin = 3073 = 193 blocks is past 160 as well, inside the d-split range 161 .. 255).  (a), (b): a second evaluation returns the
    same bits — a race between the waves of the paired loop could pass one tolerance check by luck."""
    c = dict(TRAIN[name])
    if "make" in c:
        c.update(c["make"](np.random.RandomState(11)))
    N, S = N_BWD, S4
    assert _blocks(S * N) > BWD_8W_BLOCKS and _blocks(S * N) > FWD_8W_BLOCKS and (S * N) % 16 == 4
    assert FWD_8W_BLOCKS < _blocks(N) < 256
    _set_force(monkeypatch, c.get("force"))
    X, Y, spec, state, model, zs = _build(c["specs"], N, c["DY"], M=c.get("M", 128), S=S, white=c.get("white", False),
                                          num_classes=c.get("num_classes"), seed=sum(map(ord, name)))
    _grad_check(X, Y, spec, state, model, zs, S, num_data=4 * N)
    if c.get("twice"):
        g1 = _grads(model)
        e2 = model._build_likelihood(X, Y, zs=zs, with_grad=True)
        g2 = _grads(model)
        e3 = model._build_likelihood(X, Y, zs=zs, with_grad=True)
        g3 = _grads(model)
        assert e2 == e3
        for k in g1:
            assert np.array_equal(g1[k], g2[k]) and np.array_equal(g2[k], g3[k]), k


_ELBO_D = {}


@pytest.mark.parametrize("force", ["", "last_fuse=0"])
def test_fused_last_layer_and_the_two_chains_on_769_ragged_blocks(monkeypatch, force):
    """(d) D_Y = 1, Gaussian, non-white: the last layer's Rin = 4 x 3073 = 12 292 rows = 769 row blocks > 768 with 4 live rows in the
    last one, as the fused launch (k_layer_last) and, with `last_fuse=0`, as the two 4-wave chains.  Both meet the oracle; the two
    ELBOs agree at rtol 1e-12."""
    N, S = N_BWD, S4
    assert _blocks(S * N) > BWD_8W_BLOCKS and (S * N) % 16 == 4
    _set_force(monkeypatch, force)
    X, Y, spec, state, model, zs = _build([kern_spec("rbf", 4, 1.1, 0.9)] * 2, N, 1, seed=40)
    _grad_check(X, Y, spec, state, model, zs, S, num_data=4 * N)
    _ELBO_D[force] = model._build_likelihood(X, Y, zs=zs, with_grad=True)
    if len(_ELBO_D) == 2:
        assert_allclose(_ELBO_D[""], _ELBO_D["last_fuse=0"], rtol=1e-12)


@pytest.mark.parametrize("force", ["", "adj_fuse=0"])
def test_first_layer_backward_launch_past_768_blocks(monkeypatch, force):
    """(f) S = 2, N = 12 290: the FIRST layer's backward launch has Rin = N = 12 290 -> ldA = 12 304 = 769 row blocks > 768 (rep = S),
    2 live rows in the last one — the 4-wave chain with the adjoint prologue (up_dF), and behind k_adj_prep with `adj_fuse=0`.  The
    second layer's launches have 2 x 12 290 = 24 580 rows = 1537 blocks."""
    N, S = 12290, 2
    assert _blocks(N) > BWD_8W_BLOCKS and N % 16 == 2 and _blocks(S * N) > BWD_8W_BLOCKS
    _set_force(monkeypatch, force)
    X, Y, spec, state, model, zs = _build([kern_spec("rbf", 3, 1.1, 0.5)] * 2, N, 2, S=S, seed=60)
    _grad_check(X, Y, spec, state, model, zs, S, num_data=4 * N)


# ---------------------------------------------------------------- 2. forward-only paths at 161 row blocks
FWD = [("matern52", False), ("rbf", True)]
_FWD_REF = {}


def _fwd_specs(kind):
    return [kern_spec(kind, 4, 1.1, 0.9, white_variance=0.02), kern_spec(kind, 4, 0.9, 1.0)]


def _fwd_ref(kind, white):
    """inputs and the oracle's results, computed once per variant and left unchanged"""
    key = (kind, white)
    if key not in _FWD_REF:
        N, S = N_FWD, S4
        X, Y, spec, state, model, zs = _build(_fwd_specs(kind), N, 3, white=white, seed=80 + white)
        Xs = np.random.RandomState(90 + white).randn(S * N, 4)
        om = OM.build(O.NP, spec, state)
        _FWD_REF[key] = dict(X=X, Y=Y, zs=zs, Xs=Xs, prop=OM.propagate(spec, state, X, zs, S),
                             elbo=OM.elbo(spec, state, X, Y, zs, S, num_data=4 * N), cond=om.layers[0].conditional_ND(O.NP, Xs))
    return _FWD_REF[key]


def _fwd_model(kind, white):
    return _build(_fwd_specs(kind), N_FWD, 3, white=white, seed=80 + white)[4]


@pytest.mark.parametrize("kind,white", FWD)
def test_propagate_at_161_blocks(monkeypatch, kind, white):
    """the second layer's forward launch has Rin = 4 x 641 = 2564 rows = 161 row blocks > 160 with 4 live rows in the last one; a
    forward-only call of the non-white model runs it in whitened coordinates (the WHITE 4-wave instance)"""
    N, S = N_FWD, S4
    assert _blocks(S * N) > FWD_8W_BLOCKS and (S * N) % 16 == 4
    _set_force(monkeypatch, "")
    ref = _fwd_ref(kind, white)
    model = _fwd_model(kind, white)
    Fs, Fm, Fv = model.propagate(ref["X"], S=S, zs=ref["zs"])
    Fs_o, Fm_o, Fv_o = ref["prop"]
    for l in range(2):
        assert_allclose(Fm[l], Fm_o[l], rtol=1e-9, atol=1e-10)
        assert_allclose(Fv[l], Fv_o[l], rtol=1e-9, atol=1e-10)
        assert_allclose(Fs[l], Fs_o[l], rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("kind,white", FWD)
def test_elbo_value_at_161_blocks_in_both_coordinate_forms(monkeypatch, kind, white):
    """compute_log_likelihood (Rin = 2564 = 161 row blocks > 160 on the last layer): the default form — whitened coordinates for the
    non-white model — and `white_fwd=0` on a fresh model both meet the oracle and agree with each other at rtol 1e-11"""
    N, S = N_FWD, S4
    assert _blocks(S * N) > FWD_8W_BLOCKS
    ref = _fwd_ref(kind, white)
    got = {}
    for force in ("", "white_fwd=0"):
        _set_force(monkeypatch, force)
        model = _fwd_model(kind, white)
        got[force] = model.compute_log_likelihood(ref["X"], ref["Y"], zs=ref["zs"])
        assert_allclose(got[force], ref["elbo"], rtol=1e-9)
    assert_allclose(got[""], got["white_fwd=0"], rtol=1e-11)


@pytest.mark.parametrize("kind,white", FWD)
def test_conditional_at_161_blocks_against_the_oracle_and_the_8_wave_instance(monkeypatch, kind, white):
    """layers[0].conditional_ND on 2564 test rows (Rin = 2564 = 161 row blocks > 160: the 4-wave instance) against the oracle; and
    against the same layer's result for the first 2560 rows alone (160 row blocks: the 8-wave instance) — a row's result does not
    depend on which rows share its launch — at rtol 1e-11 / atol 1e-12."""
    n = S4 * N_FWD
    assert _blocks(n) > FWD_8W_BLOCKS and _blocks(n - 4) == FWD_8W_BLOCKS and n % 16 == 4
    _set_force(monkeypatch, "")
    ref = _fwd_ref(kind, white)
    model = _fwd_model(kind, white)
    m4, v4 = model.layers[0].conditional_ND(ref["Xs"])
    mo, vo = ref["cond"]
    assert_allclose(m4, mo, rtol=1e-9, atol=1e-10)
    assert_allclose(v4, vo, rtol=1e-9, atol=1e-10)
    m8, v8 = model.layers[0].conditional_ND(ref["Xs"][:n - 4])
    print("instance against instance: max |dmean| %.3e, max |dvar| %.3e" % (np.max(np.abs(m4[:n - 4] - m8)), np.max(np.abs(v4[:n - 4] - v8))))
    assert_allclose(m4[:n - 4], m8, rtol=1e-11, atol=1e-12)
    assert_allclose(v4[:n - 4], v8, rtol=1e-11, atol=1e-12)
