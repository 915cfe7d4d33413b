"""Kernels and gradients under a joint shift of X and Z (run with -m gpu).

Every other GPU test draws its inputs around the origin, the one regime where |x|^2 + |z|^2 - 2 x.z costs nothing.  The device forms
squared distances that way on the MFMA pipe at some sites (the chains' Kuf tile, the head launch's Ku, dsdgp_gram for D <= 32) and by
direct differences at others (k_gram for D > 32, the GEMM-formulated K(Z, X), the Ku build outside the head launch), and the reverse pass
has cancelling sums of its own (the Z gradient through [X^T; 1], the lengthscale gradient, the inner layers' dX).  Here the inputs sit
at 2^6 and 2^10 from the origin, rows coincide with inducing points bit for bit, and pairs lie far enough apart for exp to underflow.

(a) model level: tests/shift_cases.py's configurations at X + c s, Z + c s against THE SAME DEVICE MODEL at c = 0 (an exact
    restatement of the same problem, which the rest of the suite holds to the oracle), every quantity within
    bar(q) = 8 max(family(q), 2^-40) of tests/shift_reference.py — the float64 oracle's own movement under the same shifts, computed
    when the test runs.  Nothing here is tuned to a device value.
(b) dsdgp_gram entrywise against the long-double matrix, with the bar of the form the width selects (expanded for D <= 32, direct
    above: derived in tests/shift_reference.py); the symmetric call exactly symmetric with one diagonal value.
    At 37 x 131 these calls reach the sub-chunk form k_gram_mfma2 (D <= 32) and k_gram (D > 32) only: the streaming form
    k_gram_mfma3 needs D <= 8 and at least 8192 tiles of 64 x 32 (gram_launch).
(c) the streaming form and the sub-chunk form of the Gram build stay bitwise equal on a shared block at offset 2^10, and 128 columns
    of the large result are held entrywise to the long-double matrix with the expanded bar.  This is the only place the streaming
    form sees the offset, and only in a library built with DSDGP_GRAM_STREAM_VALIDATED=1 (the Makefile's setting for the validated
    compiler) or run with DSDGP_GRAM_STREAM=1: otherwise both calls take the sub-chunk form and (c) compares it with itself.
(d) DSDGP_SHIFT_PROFILE=<file> writes the measured ratios (profiles/kernel_shift_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from doubly_stochastic_dgp import _lib
from tests import shift_cases as SC
from tests import shift_reference as R

pytestmark = pytest.mark.gpu

_MODEL_ROWS, _GRAM_ROWS = [], []
_PROFILE = os.environ.get("DSDGP_SHIFT_PROFILE")


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    if not _PROFILE or not (_MODEL_ROWS or _GRAM_ROWS):
        return
    with open(_PROFILE, "w") as f:
        f.write("# Kernels and gradients under a joint shift of X and Z: measured ratios (tests/test_gpu_kernel_shift.py)\n\n"
                "## Model level\n\n"
                "`device / bar`: the largest distance of the device at `X + c s, Z + c s` (four sign patterns) from the device at `c = 0`,\n"
                "over `bar = 8 max(family, 2^-40)` (1 = at the bar).  `family`: the float64 oracle's own movement with the clamped\n"
                "expansion, in units of the quantity's largest magnitude at `c = 0`.  `device / direct`: the device's movement over that of\n"
                "the float64 oracle with direct differences (recorded, not asserted: how far the device is from a form that does not\n"
                "cancel).\n\n"
                "| configuration | c | quantity | device / bar | family | device / direct |\n|---|---|---|---|---|---|\n")
        for r in _MODEL_ROWS:
            f.write("| %s | 2^%d | %s | %.3g | %.2e | %.3g |\n" % r)
        f.write("\n## dsdgp_gram\n\n"
                "Largest `|device - long double| / bar` over the entries of the 37 x 131 result (expanded-form bar for `D <= 32`,\n"
                "direct-form bar above), and the largest bar in units of `v`.  Last rows: the 128 sampled columns of the large result of the\n"
                "shared-block test, the one call that reaches the streaming form.\n\n"
                "| family | D | kind | device / bar | largest bar / v |\n|---|---|---|---|---|\n")
        for r in _GRAM_ROWS:
            f.write("| %s | %d | %s | %.3g | %.2e |\n" % r)


# ------------------------------------------------------------------------------------------------ (a) model level
_DEVICE0 = {}


def _device(name, c=0.0, pattern=0):
    cs = SC.CASES[name]
    _, _, model, Xs, arr, sh = SC.build(name, c, pattern)
    _, Fm, Fv = model.propagate(Xs, S=cs["S"], zs=arr["zs"])
    e = model._build_likelihood(Xs, arr["Y"], zs=arr["zs"], with_grad=True)
    g = model.engine().gradient_dict()
    q = {"elbo": np.array([float(e)])}
    for k in sorted(g):
        q["grad " + k] = np.asarray(g[k], dtype=np.float64).copy()
    for l in range(cs["L"]):
        fm = np.asarray(Fm[l], dtype=np.float64)
        q[f"Fmean l{l}"] = fm - sh if l < cs["L"] - 1 else fm
        q[f"Fvar l{l}"] = np.asarray(Fv[l], dtype=np.float64).copy()
    return q


@pytest.mark.parametrize("c", SC.SHIFTS, ids=lambda c: "c=2^%d" % int(np.log2(c)))
@pytest.mark.parametrize("name", list(SC.CASES))
def test_model_under_a_joint_shift_moves_no_more_than_float64_itself(monkeypatch, name, c):
    cs = SC.CASES[name]
    if cs["force"]:
        monkeypatch.setenv("DSDGP_FORCE", cs["force"])
    if name not in _DEVICE0:
        _DEVICE0[name] = _device(name)
    q0 = _DEVICE0[name]
    _, fam = R.family(name, c)
    assert set(fam) == set(q0)          # the oracle and the device name the same quantities
    bars = R.bars(name, c)
    sc = R.scales(q0)
    worst = {k: 0.0 for k in q0}
    for p in range(4):
        q = _device(name, c, p)
        for k, v in q.items():
            assert np.all(np.isfinite(v)), (k, p)
            if k.startswith("Fvar"):
                assert np.all(v >= -SC.JITTER), (k, p, float(v.min()))
        for k, m in R.moved(q, q0, sc).items():
            worst[k] = max(worst[k], m)
    direct = R.family(name, c, "direct")[1] if _PROFILE else None
    for k in q0:
        print("%s c=%g %-32s device %.3e  family %.3e  device / bar %.3g" % (name, c, k, worst[k], fam[k], worst[k] / bars[k]))
        if _PROFILE:
            _MODEL_ROWS.append((name + (" (`%s`)" % cs["force"] if cs["force"] else ""), int(np.log2(c)), k, worst[k] / bars[k], fam[k],
                                worst[k] / max(direct[k], 2.0 ** -53)))
    over = {k: worst[k] / bars[k] for k in q0 if not worst[k] <= bars[k]}
    assert not over, over


# ------------------------------------------------------------------------------------------------ (b) dsdgp_gram
def _p(t):
    return C.c_void_p(t.data_ptr())


def _spec(kind, D, ls, var, white=None):
    return _lib.KernelSpec(kind={"rbf": 0, "matern52": 1}[kind], input_dim=D, ard=1, has_white=int(white is not None), variance=var,
                           white_variance=white or 0.0, lengthscales=ls.ctypes.data_as(_lib.c_double_p))


def _gram(ctx, kind, X, X2, ls, white=None, jitter=0.0):
    n, D = X.shape
    n2 = n if X2 is None else X2.shape[0]
    ls = np.ascontiguousarray(ls, dtype=np.float64)
    dX = ctx.to_device(X)
    dX2 = None if X2 is None else ctx.to_device(X2)
    out = ctx.empty(n, n2)
    ctx.torch.cuda.current_stream().synchronize()
    _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(_spec(kind, D, ls, R.GRAM_V, white)), _p(dX), n, None if X2 is None else _p(dX2),
                                  0 if X2 is None else n2, jitter, _p(out), n2))
    ctx.sync()
    return out.cpu().numpy()


def _bar(D, bar_e, bar_d):
    return bar_e if D <= 32 else bar_d          # gram_launch: the MFMA expansion up to D = 32, k_gram's direct differences above


@pytest.mark.parametrize("D", R.GRAM_DIMS)
@pytest.mark.parametrize("fam", R.GRAM_FAMILIES)
def test_gram_entrywise_against_long_double(ctx, fam, D):
    X, X2, ls = R.gram_inputs(fam, D)
    for kind in R.GRAM_KINDS:
        K, bar_e, bar_d = R.gram_bars(kind, X, X2, ls, R.GRAM_V)
        bar = _bar(D, bar_e, bar_d)
        got = _gram(ctx, kind, X, X2, ls)
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and np.all(got <= R.GRAM_V), kind
        ratio = (np.abs(got.astype(R.LD) - K).astype(np.float64) / bar)
        print("%s D=%d %s: device / bar %.3g (largest bar %.2e v)" % (fam, D, kind, ratio.max(), bar.max() / R.GRAM_V))
        if _PROFILE:
            _GRAM_ROWS.append((fam, D, kind, float(ratio.max()), float(bar.max() / R.GRAM_V)))
        assert ratio.max() <= 1.0, (kind, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))


@pytest.mark.parametrize("D", R.GRAM_DIMS)
@pytest.mark.parametrize("fam", R.GRAM_FAMILIES)
def test_gram_symmetric_call_is_exactly_symmetric_with_one_diagonal_value(ctx, fam, D):
    """K(X2, X2) + (white + jitter) I of the 131 rows (for `coincide`: 37 rows twice, bit for bit, and once more 2^-24 away).  Exact
    symmetry, ONE diagonal value — v + (white + jitter) for RBF and, for Matern52, the float64 formula at r = 1e-6 (the 1e-12 under the
    root) plus (white + jitter), to 2 ulp — and every entry off the diagonal within the bar of the form."""
    _, X, ls = R.gram_inputs(fam, D)
    n = X.shape[0]
    white, jitter = 0.3, 1e-6
    for kind in R.GRAM_KINDS:
        Ks = _gram(ctx, kind, X, None, ls, white=white, jitter=jitter)
        assert np.array_equal(Ks, Ks.T), kind
        dg = np.diagonal(Ks)
        assert np.all(dg == dg[0]), kind
        want = float(R.kfun(kind, R.GRAM_V, np.zeros(1))[0]) + (white + jitter)
        assert abs(dg[0] - want) <= 2.0 * np.spacing(want), (kind, dg[0], want)
        K, bar_e, bar_d = R.gram_bars(kind, X, X, ls, R.GRAM_V)
        off = ~np.eye(n, dtype=bool)
        ratio = np.abs(Ks.astype(R.LD) - K).astype(np.float64)[off] / _bar(D, bar_e, bar_d)[off]
        assert ratio.max() <= 1.0, (kind, float(ratio.max()))


# ------------------------------------------------------------------------------------------------ (c) the streaming form
@pytest.mark.parametrize("kind", R.GRAM_KINDS)
def test_gram_both_forms_agree_bitwise_on_a_shared_block_at_an_offset(ctx, kind):
    """tests/test_gpu_round5.py::test_gram_both_forms_agree_bitwise_on_a_shared_block with every input 2^10 from the origin and the
    first 512 rows of X2 equal to X: a 512 x 33 000 result (streaming form) and the 512 x 4000 result of its first columns (sub-chunk
    form) are two launches of ONE tile arithmetic and carry the same bits — the clamp and the near-zero distances included.  Equal
    bits say nothing about their value, so 128 columns of the large result are also held to the long-double matrix."""
    rng = np.random.RandomState(8)
    n, n2, n2s, D = 512, 33000, 4000, 8
    off = 2.0 ** 10 * SC.signs(D)[1]
    X, X2 = rng.randn(n, D) + off, rng.randn(n2, D) + off
    X2[:n] = X
    ls = np.array([0.9])
    sp = _lib.KernelSpec(kind={"rbf": 0, "matern52": 1}[kind], input_dim=D, ard=0, has_white=0, variance=1.0, white_variance=0.0,
                         lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    dX, dX2 = ctx.to_device(X), ctx.to_device(X2)
    big, small = ctx.empty(n, n2), ctx.empty(n, n2s)
    ctx.torch.cuda.current_stream().synchronize()
    _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(sp), _p(dX), n, _p(dX2), n2, 0.0, _p(big), n2))
    _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(sp), _p(dX), n, _p(dX2), n2s, 0.0, _p(small), n2s))
    ctx.sync()
    b, s = big.cpu().numpy(), small.cpu().numpy()
    assert np.all(np.isfinite(b))
    assert np.array_equal(b[:, :n2s], s)
    # the large result entrywise on 128 columns: 32 of the rows that equal X bit for bit, 96 spread over the rest
    cols = np.concatenate([np.arange(0, n, n // 32)[:32], np.linspace(n, n2 - 1, 96).astype(np.int64)])
    K, bar_e, _ = R.gram_bars(kind, X, X2[cols], np.full(D, ls[0]), 1.0)
    ratio = np.abs(b[:, cols].astype(R.LD) - K).astype(np.float64) / bar_e
    print("streaming %s: device / bar %.3g" % (kind, ratio.max()))
    if _PROFILE:
        _GRAM_ROWS.append(("shift10, 512 x 33 000 (128 columns)", D, kind, float(ratio.max()), float(bar_e.max())))
    assert ratio.max() <= 1.0, float(ratio.max())
