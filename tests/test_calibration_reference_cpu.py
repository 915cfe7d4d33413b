"""The CPU reference of tests/test_gpu_calibration.py (tests/calibration_reference.py) pinned on its own, without a GPU: the closed-form
CRPS against the integral of (F(x) - 1[x >= y])^2 by adaptive quadrature, the quantile solver and the PIT against 10^6 direct draws from
the mixture (within the binomial sampling error of the count of draws below a point), the quantiles' order in p, the 40-digit F and f
against float64 — and the host side of the feature that needs no device: the four C-ABI entries are declared with the argument counts
of include/dsdgp.h, the scores are formed from the accumulator as documented, and every argument DGP_Base.predict_quantiles /
calibration refuse is refused before a device is asked for."""
import ctypes
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_allclose
from scipy.integrate import quad

from tests import calibration_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (1e-6, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0 - 1e-6)


def _mixture(S, seed, scale=1.0, shift=0.0, noise=0.3, items=(2, 2)):
    rng = np.random.RandomState(seed)
    mu = scale * rng.randn(S, *items) + shift
    sg = R.sigma(rng.uniform(0.01, 1.5, size=(S,) + items), noise)
    return rng, mu, sg


def _crps_by_quadrature(y, mu, sg):
    """one item: the integral of F^2 below y plus that of (1 - F)^2 above, split at every component mean"""
    F = lambda x: float(R.cdf(np.float64(x), mu, sg))
    lo, hi = float((mu - 40.0 * sg).min()), float((mu + 40.0 * sg).max())
    lo, hi = min(lo, y - 1.0), max(hi, y + 1.0)
    cuts = sorted(set([lo, hi, float(y)] + [float(m) for m in mu if lo < m < hi]))
    total = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        g = (lambda x: F(x) ** 2) if b <= y else (lambda x: (1.0 - F(x)) ** 2)
        total += quad(g, a, b, epsabs=1e-14, epsrel=1e-13, limit=400)[0]
    return total


@pytest.mark.parametrize("S,scale,shift", [(1, 1.0, 0.0), (2, 1.0, 100.0), (3, 10.0, 0.0), (17, 0.1, 0.0), (100, 1.0, 0.0)])
def test_closed_form_crps_matches_the_integral(S, scale, shift):
    rng, mu, sg = _mixture(S, 10 + S, scale, shift)
    y = shift + scale * rng.randn(2, 2) + rng.randn(2, 2)
    got = R.crps(y, mu, sg)
    for i in range(2):
        for d in range(2):
            assert_allclose(got[i, d], _crps_by_quadrature(y[i, d], mu[:, i, d], sg[:, i, d]), rtol=1e-10)
    if S == 1:
        assert_allclose(got, R.crps_single_gaussian(y, mu[0], sg[0]), rtol=1e-13)


def test_closed_form_crps_of_a_bimodal_mixture():
    """two groups of four unit-variance components at -30 and +30, targets inside a group, in the gap and outside"""
    rng = np.random.RandomState(21)
    mu = np.concatenate([-30.0 + 0.1 * rng.randn(4), 30.0 + 0.1 * rng.randn(4)])
    sg = np.ones(8)
    for y in (-29.5, 0.0, 12.0, 31.0, 80.0):
        got = float(R.crps(np.array([y]), mu[:, None], sg[:, None])[0])
        assert_allclose(got, _crps_by_quadrature(y, mu, sg), rtol=1e-10)


N_DRAWS = 10 ** 6


@pytest.fixture(scope="module")
def draws():
    """10^6 direct draws from each of four mixtures (S = 5, items 2 x 2), and the mixtures"""
    rng, mu, sg = _mixture(5, 3, scale=2.0)
    comp = rng.randint(0, 5, size=(N_DRAWS, 2, 2))
    ii, dd = np.meshgrid(np.arange(2), np.arange(2), indexing="ij")
    x = mu[comp, ii, dd] + sg[comp, ii, dd] * rng.randn(N_DRAWS, 2, 2)
    return mu, sg, x


def test_quantiles_match_direct_draws(draws):
    """the number of draws <= q_k is Binomial(n, p_k): the observed fraction within 5 standard deviations of p_k"""
    mu, sg, x = draws
    probs = (0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999)
    q = R.quantiles(mu, sg, probs)
    for k, p in enumerate(probs):
        frac = (x <= q[..., k][None]).mean(0)
        assert np.all(np.abs(frac - p) <= 5.0 * np.sqrt(p * (1.0 - p) / N_DRAWS)), (p, frac)
        # and the order statistic itself: the empirical quantile lies where F is within the same error of p
        emp = np.quantile(x, p, axis=0)
        assert np.all(np.abs(R.cdf(emp, mu, sg) - p) <= 5.0 * np.sqrt(p * (1.0 - p) / N_DRAWS) + 1.0 / N_DRAWS)


def test_pit_matches_direct_draws(draws):
    mu, sg, x = draws
    for y in (np.array([[-1.0, 0.3], [2.5, -4.0]]), mu[2], mu[0] + 3.0 * sg[0]):
        u = R.pit(y, mu, sg)
        frac = (x <= y[None]).mean(0)
        assert np.all(np.abs(frac - u) <= 5.0 * np.sqrt(u * (1.0 - u) / N_DRAWS) + 1.0 / N_DRAWS), (u, frac)


@pytest.mark.parametrize("S,scale,shift", [(1, 1.0, 0.0), (2, 10.0, 100.0), (9, 0.1, 100.0), (30, 10.0, 0.0)])
def test_quantiles_solve_their_equation_and_do_not_decrease_in_p(S, scale, shift):
    _, mu, sg = _mixture(S, 40 + S, scale, shift, noise=0.0, items=(5, 2))
    q = R.quantiles(mu, sg, PROBS)
    assert np.all(np.diff(q, axis=-1) > 0.0)
    worst = 0.0
    for i in range(5):
        for k, p in enumerate(PROBS):
            worst = max(worst, R.residual(q[i, 0, k], p, mu[:, i, 0], sg[:, i, 0]))
    assert worst < 2.0, worst      # a residual of the order of one rounding of F or of q
    if S == 1:
        from scipy.special import ndtri
        assert_allclose(q, mu[0][..., None] + sg[0][..., None] * ndtri(np.asarray(PROBS)), rtol=1e-13, atol=1e-13)


def test_quantiles_in_a_gap_and_between_spikes():
    rng = np.random.RandomState(21)
    mu = np.concatenate([-30.0 + 0.1 * rng.randn(4), 30.0 + 0.1 * rng.randn(4)])[:, None]
    q = R.quantiles(mu, np.ones_like(mu), PROBS)[0]
    assert abs(q[3]) < 25.0 and float(R.cdf(q[3:4], mu, np.ones_like(mu))[0]) == 0.5      # anywhere in the gap F = 1/2 exactly
    assert np.all(np.diff(q) > 0.0)
    mu, sg = np.array([-5.0, 5.0, 0.0])[:, None], np.array([1e-3, 1e-3, 3.0])[:, None]
    q = R.quantiles(mu, sg, PROBS)[0]
    assert np.all(np.diff(q) > 0.0) and q[3] == 0.0
    assert max(R.residual(q[k], p, mu[:, 0], sg[:, 0]) for k, p in enumerate(PROBS)) < 2.0


def test_extended_precision_versions_agree_with_float64():
    _, mu, sg = _mixture(7, 5, items=(3,))
    for x in (-2.0, 0.1, 3.0):
        for i in range(3):
            assert_allclose(float(R.cdf_mp(x, mu[:, i], sg[:, i])), R.cdf(np.full(3, x), mu, sg)[i], rtol=1e-14)
            assert_allclose(float(R.pdf_mp(x, mu[:, i], sg[:, i])), R.pdf(np.full(3, x), mu, sg)[i], rtol=1e-14)
    # far in the tail, where float64 keeps only the relative accuracy of erfc
    assert_allclose(float(R.cdf_mp(-40.0, np.zeros(1), np.ones(1))), R.cdf(np.array([-40.0]), np.zeros((1, 1)), np.ones((1, 1)))[0], rtol=1e-13)


def test_sums_and_scores():
    r = np.zeros((4, 2, 2))
    r[:, 0, 0] = [0.01, 0.3, 0.6, 0.99]
    r[:, 1, 0] = [0.04, 0.05, 0.5, 0.96]
    r[:, 0, 1] = [1.0, 2.0, 3.0, 4.0]
    r[:, 1, 1] = 0.5
    probs = (0.025, 0.05, 0.5, 0.95, 0.975)
    s = R.sums(r, probs)
    assert s.shape == (7, 2)
    assert np.array_equal(s[0], [10.0, 2.0]) and np.array_equal(s[1], [4.0, 4.0])
    assert np.array_equal(s[2:, 0], [1, 1, 2, 3, 3]) and np.array_equal(s[2:, 1], [0, 2, 3, 3, 4])
    from doubly_stochastic_dgp.dgp import calibration_scores
    for got in (R.scores(s, probs, Y_std=2.0), calibration_scores(s, probs, Y_std=2.0)):
        assert got["crps"] == 2.0 * 12.0 / 8.0 and np.array_equal(got["crps_per_output"], [5.0, 1.0])
        assert np.array_equal(got["pit_le"], s[2:] / 4.0)
        assert sorted(got["coverage"]) == pytest.approx([0.9, 0.95])
        cov = {round(k, 6): v for k, v in got["coverage"].items()}
        assert cov[0.95] == (7 - 1) / 8.0 and cov[0.9] == (6 - 3) / 8.0
    assert R.scores(s[:4], probs[:2])["coverage"] == {}


# ---------------------------------------------------------------- the host side that needs no device
def _header_arg_count(name):
    text = open(os.path.join(ROOT, "include", "dsdgp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/dsdgp.h"
    return len(m.group(1).split(","))


@pytest.mark.parametrize("name,count", [("dsdgp_mixture_quantiles", 10), ("dsdgp_mixture_calibration", 13), ("dsdgp_model_quantiles", 11),
                                        ("dsdgp_model_calibration", 13)])
def test_binding_declares_the_new_entry_points(name, count):
    from doubly_stochastic_dgp import _lib
    assert name in _lib.EXPORTED_SYMBOLS
    res, args = _lib._PROTOS[name]
    assert res is ctypes.c_int and len(args) == count == _header_arg_count(name)
    if os.path.exists(_lib.lib_path()):          # the built library exports it (dlopen needs no GPU)
        assert hasattr(ctypes.CDLL(_lib.lib_path()), name)
    assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _models():
    """built as tests/test_host_cpu.py builds its own"""
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Bernoulli, Gaussian
    rng = np.random.RandomState(0)
    X = rng.randn(20, 2)
    gauss = DGP(X, X[:, :1], X[:5], [RBF(2), RBF(2)], Gaussian())
    bern = DGP(X, np.sign(X[:, :1]), X[:5], [RBF(2), RBF(2)], Bernoulli())
    return X, gauss, bern


def test_host_validation_comes_before_the_device():
    """every refused argument raises its own error whether or not a GPU is present: nothing below touches the engine"""
    X, gauss, bern = _models()
    Y = X[:, :1]
    z_ok = [np.zeros((3, 20, 2)), np.zeros((3, 20, 1))]
    bad_probs = [(), (0.0, 0.5), (0.5, 1.0), (-0.1,), (1.5,), (float("nan"),), tuple(np.linspace(0.1, 0.9, 17)), ((0.1, 0.2), (0.3, 0.4))]
    for probs in bad_probs:
        with pytest.raises(ValueError):
            gauss.predict_quantiles(X, 3, probs=probs)
        with pytest.raises(ValueError):
            gauss.calibration(X, Y, 3, probs=probs)
        with pytest.raises(ValueError):
            bern.predict_quantiles(X, 3, probs=probs, level="f")
    with pytest.raises(ValueError, match="level"):
        gauss.predict_quantiles(X, 3, level="g")
    for kw in (dict(batch_size=0), dict(Y_std=0.0), dict(Y_std=-1.0), dict(Y_std=float("nan")), dict(zs=[None]), dict(zs=[np.zeros((3, 2)), None])):
        with pytest.raises(ValueError):
            gauss.predict_quantiles(X, 3, **kw)
        with pytest.raises(ValueError):
            gauss.calibration(X, Y, 3, **kw)
    for S in (0, -2):
        with pytest.raises(ValueError):
            gauss.predict_quantiles(X, S)
        with pytest.raises(ValueError):
            gauss.calibration(X, Y, S, zs=z_ok)
    with pytest.raises(ValueError):
        gauss.calibration(X, Y[:-1], 3)                      # row counts
    with pytest.raises(ValueError):
        gauss.calibration(X, np.zeros((20, 2)), 3)           # outputs of the last layer
    with pytest.raises(ValueError):
        gauss.predict_quantiles(X[:0], 3)
    with pytest.raises(ValueError):
        gauss.predict_quantiles(X[:, 0], 3)
    # the predictive y of a non-Gaussian likelihood is no Gaussian mixture
    with pytest.raises(NotImplementedError):
        bern.predict_quantiles(X, 3)
    with pytest.raises(NotImplementedError):
        bern.predict_quantiles(X, 3, level="y")
    with pytest.raises(NotImplementedError):
        bern.calibration(X, np.sign(Y), 3)
    with pytest.raises(NotImplementedError):
        bern.likelihood.mixture_quantiles(np.zeros((2, 3, 1)), np.ones((2, 3, 1)), (0.5,))
    with pytest.raises(NotImplementedError):
        bern.likelihood.mixture_calibration(np.zeros((2, 3, 1)), np.ones((2, 3, 1)), np.zeros((3, 1)), (0.5,))
    with pytest.raises(ValueError):
        gauss.likelihood.mixture_quantiles(np.zeros((2, 3, 1)), np.ones((2, 3, 1)), (0.5,), level="g")
    with pytest.raises(ValueError):
        gauss.likelihood.mixture_quantiles(np.zeros((2, 3, 1)), np.ones((2, 3, 1)), (0.0,))
    with pytest.raises(ValueError):
        gauss.likelihood.mixture_calibration(np.zeros((2, 3, 1)), np.ones((2, 3, 1)), np.zeros((3, 1)), ())


def test_valid_arguments_reach_the_device_or_its_absence():
    """with valid arguments the call goes on to the engine: without a GPU that is the library's "no CPU fallback" error"""
    import torch
    from doubly_stochastic_dgp import _lib
    X, gauss, bern = _models()
    calls = [lambda: gauss.predict_quantiles(X, 3), lambda: bern.predict_quantiles(X, 3, level="f"),
             lambda: gauss.calibration(X, X[:, :1], 3)["pit_le"]]
    for call, shape in zip(calls, [(20, 1, 3), (20, 1, 3), (7, 1)]):
        if torch.cuda.is_available():
            assert call().shape == shape
        else:
            with pytest.raises(_lib.DsdgpError, match="no CPU fallback"):
                call()
