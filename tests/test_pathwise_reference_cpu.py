"""Conditions on the reference of the pathwise draws alone (tests/pathwise_reference.py): what the GPU tests compare the device with has
to be right before anything is compared with it."""
import numpy as np
import pytest

from tests import pathwise_cases as PC
from tests import pathwise_reference as PR


@pytest.mark.parametrize("kind,ard", [("rbf", False), ("rbf", True), ("matern52", False), ("matern52", True)])
def test_the_basis_kernel_is_the_kernel_within_its_standard_errors(kind, ard):
    """K^ at L = 16384 is within 5 of its own standard errors of K on a fixed point set; the standard error of an entry is the spread of
    its L terms s2 cos(theta_j(x) - theta_j(x')) over sqrt(L)"""
    rng = np.random.default_rng(11)
    D, L, n = 3, 16384, 12
    ls = np.array([0.7, 1.1, 1.6]) if ard else np.array([0.9])
    X = rng.standard_normal((n, D))
    Om = PR.sample_basis(kind, D, L, ls, rng)
    th = X @ Om
    terms = 1.3 * np.cos(th[:, None, :] - th[None, :, :])             # (n, n, L)
    Khat, se = terms.mean(axis=-1), terms.std(axis=-1, ddof=1) / np.sqrt(L)
    K = PR.kernel(kind, X, X, 1.3, ls, np.float64)
    off = ~np.eye(n, dtype=bool)
    worst = np.max(np.abs(Khat - K)[off] / se[off])
    print(f"{kind} ard={ard}: worst |K^ - K| / se = {worst:.3g}")
    assert worst <= 5.0
    assert np.allclose(np.diag(Khat), 1.3, rtol=0, atol=1e-12)         # the paired form: Var f0(x) = s2 exactly


@pytest.mark.parametrize("name", ("n16", "n17", "qnull", "d33"))
def test_a_draw_passes_through_the_inducing_outputs(name):
    """f(z_m) + (White variance + jitter) v_m = u_m + m(z_m), in long double: K(Z, Z) v = u - f0(Z) - (White variance + jitter) v"""
    c = PC.inputs(name)
    v, _ = PC.weights(name)
    f, _ = PR.evaluate(c["kind"], c["Z"], c["Omega"], c["origin"], c["Wc"], c["Ws"], c["Z"], v, c["variance"], c["ls"], None)
    Lu = PR.cholesky(PR.ku(c["kind"], c["Z"], c["variance"], c["ls"], c["white_var"], c["jitter"]))
    eps = np.zeros((c["S"], c["M"], c["DO"])) if c["q_sqrt"] is None else c["eps"]
    u, umag = PR.inducing_draws(Lu, c["q_mu"], c["q_sqrt"], eps, c["white"])
    lhs = f + (PR.LD(c["white_var"] or 0.0) + PR.LD(c["jitter"])) * v
    scale = np.max(np.abs(u)) + np.max(np.abs(v))
    assert float(np.max(np.abs(lhs - u))) <= 1e-13 * float(scale) * c["M"]


def test_the_twins_moments_are_the_closed_form_given_the_basis():
    """The moment-test configuration (tests/pathwise_cases.py), the device's own normals replayed through Philox: the float64 twin's
    sample mean and covariance over T = 4096 draws are within 4 standard errors of the exact conditional mean and of the closed-form
    covariance given the basis (the GPU bar is 5).  Seed 4: mean 1.61, covariance 1.95 standard errors; seeds 0 .. 5 gave at most 2.70
    and 2.99."""
    c, seed = PC.moment_config(), PC.MOMENT_SEED
    Om = PR.sample_basis(c["kind"], 2, PC.MOMENT_L, c["ls"], np.random.default_rng(seed))
    Wc, Ws, eps = PR.replay_normals(seed, 0, PC.MOMENT_T, PC.MOMENT_L, 16, 1)
    args = (c["variance"], c["ls"])
    V, _ = PR.weights(c["kind"], c["Z"], Om, c["origin"], Wc, Ws, c["q_mu"], c["q_sqrt"], eps, *args, c["white_var"], c["jitter"],
                      c["white"], np.float64)
    F, _ = PR.evaluate(c["kind"], c["X"], Om, c["origin"], Wc, Ws, c["Z"], V, *args, None, np.float64)
    rm, rc = PC.moment_ratios(F[:, :, 0], Om)
    print(f"twin moments: mean {rm:.3g}, covariance {rc:.3g} standard errors")
    assert rm <= 4.0 and rc <= 4.0
    # the exact mean is the layer's conditional mean k(X, Z) Ku^-1 q_mu
    mean, _ = PR.moments_given_basis(c["kind"], c["X"], Om, c["origin"], c["Z"], c["q_mu"], c["q_sqrt"], *args, None, c["jitter"], False)
    Ku = PR.ku(c["kind"], c["Z"], *args, None, c["jitter"], np.float64)
    want = PR.kernel(c["kind"], c["X"], c["Z"], *args, np.float64) @ np.linalg.solve(Ku, c["q_mu"])
    assert np.allclose(mean.astype(np.float64), want, rtol=1e-9, atol=1e-12)


def test_the_theta_cases_stand_on_the_sides_of_the_switch_they_name():
    """the two-constant reduction serves |theta| < 4096 (PW_FAST_MAX of csrc/pathwise_plan.hpp)"""
    for name, lo in (("theta_lo", True), ("theta_hi", False)):
        c = PC.inputs(name)
        th = np.abs((np.asarray(c["X"]).reshape(-1, c["D"]) - c["origin"]) @ c["Omega"])
        print(name, "max |theta| =", th.max(), "share below 4096 =", np.mean(th < 4096.0))
        assert (th.max() < 4096.0) if lo else (th.max() > 1e4 and np.any(th < 4096.0) and np.any(th >= 4096.0))


def test_the_twin_is_close_to_the_truth_on_every_case():
    """the float64 sequence is a usable yardstick: within 2^-40 of mag of the truth wherever both are finite"""
    for name in PC.NAMES:
        (tr, mag), (tw, _) = PC.evaluate(name), PC.evaluate(name, np.float64)
        ok = np.isfinite(tr.astype(np.float64))
        assert np.all(np.abs(tw - tr)[ok] <= 2.0 ** -40 * mag[ok]), name
        if "nan" in PC.CASES[name][-1]:
            assert np.all(~ok[:, PC.NAN_ROW]) and np.all(np.delete(ok, PC.NAN_ROW, axis=1))
