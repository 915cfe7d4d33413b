"""The CPU reference of tests/test_gpu_factor_direct.py held to its own bars (no GPU): the three inducing-point families at M = 32 and
128 through LAPACK (dpotrf, then substitution and dtrtri), every measure of tests/factor_reference.py with the device's multiplier set to
1.  If the reference needed the device's margin itself, a bar of the GPU test would say nothing about the kernels."""
import numpy as np
import pytest

from tests import factor_reference as R


KINDS, SIZES = ["rbf", "matern52"], [32, 128]


@pytest.fixture(scope="module", autouse=True)
def truths():
    """all 40-digit factorisations of this module at once, in worker processes (as the GPU test does)"""
    R.truth_many([R.reference_ku(*R.family_case(f, M, k), 1e-6) for f in R.FAMILIES for M in SIZES for k in KINDS])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_lapack_meets_every_bar_with_multiplier_one(family, M, kind):
    Z, spec = R.family_case(family, M, kind)
    Ku = R.reference_ku(Z, spec, 1e-6)
    assert np.array_equal(Ku, Ku.T)
    ref = R.reference_measures(Ku)
    n = M
    print(f"{family} {kind} M={M} cond={ref['cond']:.2e} factor={ref['factor'] / (1e-14 * n):.3f} of its bar, inverse residuals "
          f"sub {ref['left_sub']:.3f}/{ref['right_sub']:.3f} tri {ref['left_tri']:.3f}/{ref['right_tri']:.3f} kinv {ref['kinv_sub']:.3f}/{ref['kinv_tri']:.3f}")
    assert ref["factor"] <= R.factor_bar(n)
    # multiplier 1: the bar of a scaled measure is then max(1.0, the larger of the two CPU values).  The two textbook inverses differ
    # widely per side (substitution solves L X = I: its RIGHT residual obeys |L X - I| <= gamma_n |L||X|, i.e. <= 1 here, its left one
    # is bounded by nothing of the kind), which is why the device's bar is relative to the larger one and not a constant.
    for side in ("left", "right", "congr", "kinv"):
        for how in ("_sub", "_tri"):
            assert 0.0 < ref[side + how] <= R.device_bar(ref[side], n, factor=1.0), (side, how)
        assert ref[side] <= R.DEVICE_FACTOR          # the reference itself stays inside what the floor of 1.0 grants the device
    assert ref["right_sub"] <= 1.0
    # Ku^-1 = X^T X: two sums of the same products in a possibly different order
    for X in (ref["X_sub"], ref["X_tri"]):
        assert R.kinv_asymmetry(X.T @ X) <= n * R.EPS
    # forward error against the 40-digit truth: finite, and far below cond x eps on the ill-conditioned families (so a "cond x eps" bar
    # would hide a lot: the GPU test bounds the device by a multiple of THIS number instead)
    Lt, Xt = R.truth(Ku)
    assert float(np.max(np.abs(R.xprod(Lt, Lt.T, a_lower=True) - Ku))) <= 4 * R.EPS * np.max(Ku)      # the truth reproduces Ku to its rounding
    fe_L = R.forward_error(ref["L"], Lt)
    fe_X = max(R.forward_error(ref["X_sub"], Xt), R.forward_error(ref["X_tri"], Xt))
    print(f"   forward error L {fe_L:.2e} X {fe_X:.2e}  (cond x eps = {ref['cond'] * R.EPS:.1e})")
    assert 0.0 < fe_L <= max(64 * R.EPS, 0.1 * ref["cond"] * R.EPS)
    assert 0.0 < fe_X <= max(64 * R.EPS, ref["cond"] * R.EPS)


def test_measures_notice_a_wrong_inverse():
    """the measures are not blind: one entry of X off by 1e-12 relative, one Newton step's worth of error in a pivot"""
    Z, spec = R.family_case("spread", 50)
    Ku = R.reference_ku(Z, spec, 1e-6)
    ref = R.reference_measures(Ku, with_kinv=False)
    X = ref["X_tri"].copy()
    i, j = np.unravel_index(np.argmax(np.abs(np.tril(X, -1))), X.shape)
    X[i, j] *= 1.0 + 1e-11
    l, r = R.inverse_residuals(X, ref["L"])
    assert max(l, r) > R.device_bar(max(ref["left"], ref["right"]), 50)
    L = ref["L"].copy()
    L[:, 7] *= 1.0 + 1e-11                       # a pivot's reciprocal square root short of one Newton step
    assert R.factor_backward(L, Ku) > R.factor_bar(50)


def test_float64_products_from_1024_carry_their_slack():
    assert R.product_slack(1023) == 0.0 and R.product_slack(1024) == 1.0
    assert R.factor_bar(1024) == 1e-14 * 1024 + 1024 * R.EPS
    rng = np.random.RandomState(0)
    A, B = np.tril(rng.randn(70, 70)), rng.randn(70, 70)
    assert np.max(np.abs(R.xprod(A, B, a_lower=True) - R.xprod(A, B))) == 0.0
    assert R.xprod(A, B).dtype == np.longdouble
