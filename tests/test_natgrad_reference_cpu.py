"""tests/natgrad_reference.py held to its own claims, without a GPU: the longdouble step against 40 digits, the closed form of the
quadratic family, the conditions every (family, M, gamma) of tests/test_gpu_natgrad_direct.py relies on, and the two float64
comparators against each other's bars."""
import numpy as np
import pytest

from tests import factor_reference as R
from tests import natgrad_reference as NG

from tests.natgrad_cases import CASES, REFUSED_M, case_inputs

# every (T family, M, D_out, gradient family, gamma) of the GPU table
CPU_CASES = sorted({(c.t_family, c.M, c.D_out, c.g_family, c.gamma) for c in CASES})


@pytest.mark.parametrize("M", [9, 33, 48])
def test_longdouble_step_against_40_digits(M):
    """numpy.longdouble (64-bit mantissa) against mpmath at 40 digits, same formulas: 1e-17 relative to the largest entry"""
    for tf, gf, gamma in (("dense", "generic", 0.1), ("dense_scaled", "quad", 1.0), ("init_prior", "quad", 0.1)):
        if tf == "init_prior" and M > 9:
            continue            # cond(A) grows with M on this family: longdouble itself is no longer at 1e-17 there
        q_mu, q_sqrt = NG.t_family(tf, M, 2)
        g_mu, g_sqrt = NG.g_family(gf, q_mu, q_sqrt)
        mu, sq, A, _ = NG.step_ld(q_mu, q_sqrt, g_mu, g_sqrt, gamma)
        mu_t, sq_t, A_t = NG.step_truth(q_mu, q_sqrt, g_mu, g_sqrt, gamma)
        for name, a, b in (("q_mu+", mu, mu_t), ("q_sqrt+", sq, sq_t), ("A", A, A_t)):
            err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
            print(f"M={M} {tf}/{gf} gamma={gamma}: {name} {err:.2e}")
            assert err <= 1e-17, (M, tf, gf, name, err)


@pytest.mark.parametrize("M", [20, 100])
@pytest.mark.parametrize("tf", ["dense", "dense_scaled"])
def test_quad_closed_form_at_gamma_one(M, tf):
    """quad, gamma = 1: A = S^-1 + W and m+ = A^-1 (S^-1 m + W m*), formed here from W and m* themselves, not through the gradient.
    The step only sees the gradient rounded to float64 — g_sqrt = tril(W T) and g_mu = W (m - m*) computed in float64 carry M eps |W||T|
    and M eps |W||m - m*| — and maps it through T^-T . T^-1 and A^-1: the two results agree to 8 M eps cond(T)^2 cond(A) relative, no
    better (about 1e-10 on these well-conditioned families)."""
    q_mu, q_sqrt = NG.t_family(tf, M, 2)
    g_mu, g_sqrt = NG.g_family("quad", q_mu, q_sqrt)
    W, mstar = NG.quad_terms(q_mu)
    mu, sq, A, _ = NG.step_ld(q_mu, q_sqrt, g_mu, g_sqrt, 1.0)
    for d in range(2):
        Tinv = NG._tri_inverse_ld(np.asarray(q_sqrt[d], dtype=R.LD))
        Sinv = Tinv.T @ Tinv
        Wd = np.asarray(W[d], dtype=R.LD)
        A_cf = Sinv + Wd
        tol = 8 * M * R.EPS * np.linalg.cond(q_sqrt[d]) ** 2 * np.linalg.cond(np.asarray(A_cf, dtype=np.float64))
        assert tol < 1e-9
        assert float(np.max(np.abs(A[d] - A_cf)) / np.max(np.abs(A_cf))) <= tol
        Linv = NG._tri_inverse_ld(NG._cholesky_ld(A_cf))
        m_cf = Linv.T @ (Linv @ (Sinv @ np.asarray(q_mu[:, d], dtype=R.LD) + Wd @ np.asarray(mstar[:, d], dtype=R.LD)))
        err = float(np.max(np.abs(mu[:, d] - m_cf)) / np.max(np.abs(m_cf)))
        print(f"M={M} {tf} d={d}: |m+ - closed form| = {err:.2e} (tol {tol:.2e})")
        assert err <= tol
        # T+ T+^T is A^-1
        assert float(np.max(np.abs(sq[d] @ sq[d].T @ A_cf - np.eye(M)))) <= tol


@pytest.fixture(scope="module")
def filled():
    NG.prefill([case_inputs(tf, M, D, gf) + (gamma,) for tf, M, D, gf, gamma in CPU_CASES])


@pytest.mark.parametrize("tf,M,D_out,gf,gamma", CPU_CASES, ids=[f"{t}-M{M}-D{D}-{g}-g{gm:g}" for t, M, D, g, gm in CPU_CASES])
def test_family_conditions_and_float64_comparators(filled, tf, M, D_out, gf, gamma):
    """A_ld factors in longdouble (step_ld raises otherwise), both float64 comparators give finite, exactly structured results and
    each meets the bar that the OTHER one sets (8 x its value, floor 1.0): the two orders of the same arithmetic are within the margin
    the device is given over them."""
    q_mu, q_sqrt, g_mu, g_sqrt = case_inputs(tf, M, D_out, gf)
    ref, cpu = NG.cpu_measures(q_mu, q_sqrt, g_mu, g_sqrt, gamma)
    for name, step in (("oracle", NG.step_oracle), ("reversed", NG.step_f64_reversed)):
        mu, sq = step(q_mu, q_sqrt, g_mu, g_sqrt, gamma)
        assert np.all(np.isfinite(mu))
        NG.check_structure(sq, f"{name} {tf} M={M}")
    print({k: (f"{cpu['oracle'][k]:.3g}", f"{cpu['reversed'][k]:.3g}") for k in NG.MEASURES})
    bars = NG.bars(cpu, M)
    for k in NG.MEASURES:
        for name in ("oracle", "reversed"):
            assert cpu[name][k] <= bars[k]
    # the device's order of operations (one factorisation, m+ = T+ (T+^T theta1)) is backward stable where the oracle's explicit S+
    # is not: it meets the oracle's bar on every measure
    for k in NG.MEASURES:
        assert cpu["reversed"][k] <= R.device_bar(cpu["oracle"][k], M), (k, cpu["reversed"][k], cpu["oracle"][k])


def test_benign_families_are_benign(filled):
    """every family but init_prior: the float64 comparators are within n eps of the longdouble step (scaled measures below 1)"""
    for tf, M, D_out, gf, gamma in CPU_CASES:
        if tf == "init_prior" or M >= 1024:
            continue
        ref, cpu = NG.cpu_measures(*case_inputs(tf, M, D_out, gf), gamma)
        for name in cpu:
            for k in NG.MEASURES:
                assert cpu[name][k] <= 1.0, (tf, M, gf, name, k, cpu[name][k])


@pytest.mark.parametrize("M", REFUSED_M)
def test_refused_case_is_indefinite(M):
    """quad with W replaced by -5 W, gamma = 1, on dense: A = S^-1 - 5 W has eigenvalues of both signs in every output"""
    q_mu, q_sqrt, g_mu, g_sqrt = case_inputs("dense", M, 2, "quad", w_scale=-5.0)
    A = NG.assemble_ld(q_mu, q_sqrt, g_mu, g_sqrt, 1.0)
    for d in range(2):
        ev = np.linalg.eigvalsh(np.asarray(A[d], dtype=np.float64))
        assert ev[0] < -1e-3 * np.abs(ev).max() and ev[-1] > 1e-3 * np.abs(ev).max(), (M, d, ev[0], ev[-1])
    with pytest.raises(NG.NotSPD):
        NG.step_ld(q_mu, q_sqrt, g_mu, g_sqrt, 1.0)
