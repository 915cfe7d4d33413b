"""The references of tests/test_gpu_kernel_shift.py meet the conditions that make a pass on the device mean something
(tests/shift_reference.py, tests/shift_cases.py): conditions on the float64 oracle and on numpy alone, no device value anywhere."""
import numpy as np
import pytest

from oracle import dgp_oracle as O
from tests import shift_cases as SC
from tests import shift_reference as R

ALL_CASES = list(SC.CASES)


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_shifted_problem_is_the_unshifted_one_bit_for_bit(name):
    cs = SC.CASES[name]
    arr = SC.arrays(name)
    assert np.all(np.abs(arr["X"]) < 8) and np.all(np.abs(arr["Z"]) < 8)
    for a in (arr["X"], arr["Z"]):
        assert np.array_equal(np.round(a / SC.GRID) * SC.GRID, a)
    assert np.array_equal(arr["Z"][:cs["coincide"]], arr["X"][:cs["coincide"]])
    assert all(np.all((l >= 0.7) & (l <= 1.3)) for l in arr["ls"])
    _, state0, _, X0, _, _ = SC.build(name)
    assert np.array_equal(X0, arr["X"])
    for c in SC.SHIFTS:
        for p in range(4):
            _, state, _, Xs, _, sh = SC.build(name, c, p)
            assert np.all(np.abs(sh) == c)
            assert np.array_equal(Xs - sh, arr["X"])
            for l in range(cs["L"]):
                assert np.array_equal(state[f"l{l}.Z"] - sh, state0[f"l{l}.Z"]), l
            for k in state:             # and nothing else differs
                if not k.endswith(".Z"):
                    assert np.array_equal(state[k], state0[k]), k


def test_the_upstream_form_is_why_the_family_is_clamped():
    """No clamp and no exact diagonal: at c = 2^6 the expansion leaves r^2 < -1e-12 on the diagonal of K(Z, Z), Matern52's root goes
    negative and the kernel value is not a number — the reference cannot supply one there, the clamped variant can."""
    name = "5_m150"
    arr = SC.arrays(name)
    Z = arr["Z"] + SC.shift_vector(name, 2.0 ** 6, 0)
    up = O.Kern("matern52", Z.shape[1], variance=SC.VARIANCE, lengthscales=arr["ls"][0], ARD=True)
    assert np.diagonal(up._sqdist(O.NP, Z, None)).min() < -1e-12
    with np.errstate(invalid="ignore"):
        assert not np.all(np.isfinite(np.diagonal(up.K(O.NP, Z))))
    cl = O.Kern("matern52", Z.shape[1], variance=SC.VARIANCE, lengthscales=arr["ls"][0], ARD=True, sqdist="clamped")
    Kc = cl.K(O.NP, Z)
    assert np.all(np.isfinite(Kc)) and np.all(np.diagonal(cl._sqdist(O.NP, Z, None)) == 0.0)
    assert np.all(np.diagonal(Kc) == Kc[0, 0])


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_family_meets_its_conditions(name):
    for c in SC.SHIFTS:
        members, fam = R.family(name, c)
        assert all(np.isfinite(v) for m in members for v in m.values()), c
        for k in fam:                   # no member stands alone: each within 8 x the largest of the other three
            vals = [m[k] for m in members]
            for i in range(4):
                assert vals[i] <= 8.0 * max(vals[:i] + vals[i + 1:]), (c, k, vals)
    _, fam = R.family(name, SC.SHIFTS[-1])
    for k, v in fam.items():
        assert v < 1e-6, (k, v)         # a pass within 8 x this still pins six digits of every block
        if k.endswith(".Z") or k.endswith("lengthscales_raw"):
            assert v > R.FLOOR, (k, v)  # the bar of these blocks is the family, not the floor
    bars = R.bars(name, SC.SHIFTS[-1])
    assert all(bars[k] == 8.0 * max(fam[k], 2.0 ** -40) for k in fam)


@pytest.mark.parametrize("name", ["1_head_chain", "7_wide_d80"])
def test_direct_differences_move_orders_less(name):
    """Recorded beside the family, never a bar: the movement is the expansion's, not the model's."""
    _, fam = R.family(name, SC.SHIFTS[-1])
    _, famd = R.family(name, SC.SHIFTS[-1], "direct")
    assert max(famd.values()) < 1e-2 * max(fam.values())


def _half_bar(kind, D, X, X2, ls, off_diagonal=False):
    """The float64 numpy version of the form dsdgp_gram takes at this width, within half that form's bar on every entry."""
    K, bar_e, bar_d = R.gram_bars(kind, X, X2, ls, R.GRAM_V)
    assert np.all(np.isfinite(bar_e)) and np.all(np.isfinite(bar_d)) and np.all(bar_e > 0) and np.all(bar_d > 0)
    if D <= 32:                         # the expanded form; where it runs its bar still pins six digits
        got, bar = R.gram_expanded_f64(kind, X, X2, ls, R.GRAM_V), bar_e
        assert bar_e.max() <= 1e-6 * R.GRAM_V
    else:                               # k_gram's direct differences: the bar is derived for, and claimed at, D > 32 only
        got, bar = R.gram_direct_f64(kind, X, X2, ls, R.GRAM_V), bar_d
    ratio = np.abs(got.astype(R.LD) - K).astype(np.float64) / bar
    if off_diagonal:                    # (the device's diagonal is exact by construction and asserted as such)
        ratio = ratio[~np.eye(X.shape[0], dtype=bool)]
    assert ratio.max() <= 0.5, float(ratio.max())
    return K


@pytest.mark.parametrize("kind", R.GRAM_KINDS)
@pytest.mark.parametrize("D", R.GRAM_DIMS)
@pytest.mark.parametrize("fam", R.GRAM_FAMILIES)
def test_gram_bars_hold_numpy_float64_with_a_factor_two_to_spare(fam, D, kind):
    """Each bar at the widths where dsdgp_gram takes its form (expanded up to D = 32, direct above), on the K(X, X2) of the
    entrywise test and on the K(X2, X2) of the symmetric call."""
    X, X2, ls = R.gram_inputs(fam, D)
    K = _half_bar(kind, D, X, X2, ls)
    _half_bar(kind, D, X2, X2, ls, off_diagonal=True)
    if fam == "coincide":               # the bit-equal pairs are at r = 0 exactly, the next rows 2^-24 per coordinate away
        n = R.GRAM_N
        assert np.array_equal(X2[:n], X) and np.array_equal(X2[n:2 * n] - X, np.full_like(X, 2.0 ** -24))
    if fam == "far":                    # across the denormals and into exp's underflow (RBF), tiny but normal for Matern52
        k64 = K.astype(np.float64)
        if kind == "rbf":
            assert (k64 == 0.0).any() and ((k64 > 0.0) & (k64 < 2.2e-308)).any() and (k64 >= 2.2e-308).any()
        else:
            assert 0.0 < k64.max() < 1e-30
