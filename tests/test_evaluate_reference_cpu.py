"""The CPU reference of tests/test_gpu_evaluate.py (tests/evaluate_reference.py) pinned on its own, without a GPU: the Gaussian mixture's
mean and variance against the sample moments of a large direct draw from the mixture, its log density against log of the averaged
scipy.stats.norm.pdf, the edge cases the device kernel has to meet (one component; a component 800 nats below the best), the scores
against demos/run_regression.py:119-123 taken literally — and the host side of the feature that needs no device: the two C-ABI entries
are declared with the argument counts of include/dsdgp.h, and every likelihood maps to its (kind, p0, p1)."""
import ctypes
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_allclose
from scipy.stats import norm

from tests import evaluate_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gauss_case(S=5, N=3, D=2, seed=0):
    rng = np.random.RandomState(seed)
    mean, var = rng.randn(S, N, D), rng.uniform(0.05, 1.5, size=(S, N, D))
    Y = rng.randn(N, D)
    return rng, mean, var, Y, 0.3


def test_gaussian_mixture_moments_match_a_direct_draw():
    rng, mean, var, Y, s2 = _gauss_case()
    logp, E, V = R.gaussian_components(mean, var, Y, s2)
    rows = R.mixture_rows(logp, E, V)
    S, N, D = mean.shape
    n = 400000
    comp = rng.randint(0, S, size=(n, N, D))
    ii, dd = np.meshgrid(np.arange(N), np.arange(D), indexing="ij")
    y = E[comp, ii, dd] + np.sqrt(V[comp, ii, dd]) * rng.randn(n, N, D)
    m, v = y.mean(0), y.var(0)
    # Monte-Carlo accuracy: five standard errors of the sample mean / the sample variance (fourth central moment from the sample)
    m4 = ((y - m) ** 4).mean(0)
    assert np.all(np.abs(m - rows[..., 0]) <= 5.0 * np.sqrt(v / n))
    assert np.all(np.abs(v - rows[..., 1]) <= 5.0 * np.sqrt((m4 - v ** 2) / n))
    assert np.all(rows[..., 1] > V.mean(0) - 1e-12)          # total variance >= the mean of the component variances


def test_gaussian_log_density_is_log_of_the_averaged_pdf():
    _, mean, var, Y, s2 = _gauss_case(S=7, N=11, D=3, seed=1)
    logp, E, V = R.gaussian_components(mean, var, Y, s2)
    rows = R.mixture_rows(logp, E, V)
    assert_allclose(rows[..., 2], np.log(norm.pdf(Y[None], mean, np.sqrt(var + s2)).mean(0)), rtol=1e-12)


def test_single_component_and_far_components():
    _, mean, var, Y, s2 = _gauss_case(S=1, N=6, D=2, seed=2)
    logp, E, V = R.gaussian_components(mean, var, Y, s2)
    rows = R.mixture_rows(logp, E, V)
    assert np.array_equal(rows[..., 0], mean[0]) and np.array_equal(rows[..., 2], logp[0])
    assert_allclose(rows[..., 1], var[0] + s2, rtol=1e-13)
    # a component 800 nats below the best one contributes nothing: l = best - log S
    logp = np.array([[[-3.0]], [[-803.0]], [[-1e5]]])
    rows = R.mixture_rows(logp, np.zeros((3, 1, 1)), np.ones((3, 1, 1)))
    assert rows[0, 0, 2] == -3.0 - np.log(3.0)


def test_sums_and_scores_match_run_regression_literally():
    _, mean, var, Y, s2 = _gauss_case(S=4, N=23, D=1, seed=3)
    logp, E, V = R.gaussian_components(mean, var, Y, s2)
    rows = R.mixture_rows(logp, E, V)
    s = R.sums(rows, Y)
    assert s.shape == (3, 1) and s[2, 0] == 23.0
    for Y_std in (1.0, 2.5):
        got = R.scores(s, Y_std=Y_std)
        err, nll = R.run_regression_scores(E, V, Y, Y_std)
        assert_allclose(got["rmse"], err, rtol=1e-13)
        assert_allclose(got["log_density"], nll, rtol=1e-12)
    # several outputs: per-output sums, the overall RMSE over rows and outputs
    _, mean, var, Y, s2 = _gauss_case(S=3, N=9, D=4, seed=4)
    rows = R.mixture_rows(*R.gaussian_components(mean, var, Y, s2))
    s = R.sums(rows, Y)
    assert_allclose(s[0], [sum((Y[i, d] - mean[:, i, d].mean()) ** 2 for i in range(9)) for d in range(4)], rtol=1e-13)
    assert_allclose(R.scores(s)["rmse"], R.run_regression_scores(mean, var + s2, Y, 1.0)[0], rtol=1e-13)


def test_multiclass_argmax_takes_the_lowest_index_on_ties():
    P = np.array([[[0.4, 0.4, 0.2], [0.1, 0.45, 0.45]], [[0.4, 0.4, 0.2], [0.1, 0.45, 0.45]]])      # (S=2, N=2, K=3)
    logp = np.log(np.array([[[0.4], [0.45]], [[0.4], [0.45]]]))
    rows = R.mixture_rows(logp, P, P - P ** 2)
    assert rows.shape == (2, 3, 3) and np.all(rows[0, :, 2] == rows[0, 0, 2])
    assert R.multiclass_sums(rows, np.array([[0.0], [1.0]]))[0, 0] == 0.0
    assert R.multiclass_sums(rows, np.array([[1.0], [2.0]]))[0, 0] == 2.0
    s = R.multiclass_sums(rows, np.array([[1.0], [1.0]]))
    assert s[0, 0] == 1.0 and s[2, 0] == 2.0 and np.all(s[:, 1:] == 0.0)
    assert R.scores(s, multiclass=True)["error_rate"] == 0.5


# ---------------------------------------------------------------- the host side that needs no device
def _header_arg_count(name):
    text = open(os.path.join(ROOT, "include", "dsdgp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/dsdgp.h"
    return len(m.group(1).split(","))


@pytest.mark.parametrize("name,count", [("dsdgp_eval_mixture", 13), ("dsdgp_model_evaluate", 11)])
def test_binding_declares_the_new_entry_points(name, count):
    from doubly_stochastic_dgp import _lib
    assert name in _lib.EXPORTED_SYMBOLS
    res, args = _lib._PROTOS[name]
    assert res is ctypes.c_int and len(args) == count == _header_arg_count(name)
    if os.path.exists(_lib.lib_path()):          # the built library exports it (dlopen needs no GPU)
        assert hasattr(ctypes.CDLL(_lib.lib_path()), name)


def test_evaluate_is_public_and_every_likelihood_maps_to_its_kind():
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.dgp import DGP_Base
    from doubly_stochastic_dgp.gpflow_compat import Bernoulli, Beta, Exponential, Gamma, Gaussian, MultiClass, Poisson, StudentT
    from doubly_stochastic_dgp.utils import BroadcastingLikelihood
    assert callable(DGP_Base.evaluate)
    want = [(Gaussian(variance=0.25), (_lib.LIK_GAUSSIAN, 0.25)), (MultiClass(4), (_lib.LIK_MULTICLASS, 1.0)),
            (Bernoulli(), (_lib.LIK_BERNOULLI, 1.0)), (Poisson(binsize=0.8), (_lib.LIK_POISSON, 1.0)),
            (Exponential(), (_lib.LIK_EXPONENTIAL, 1.0)), (StudentT(1.3, 3.0), (_lib.LIK_STUDENT_T, 1.3)),
            (Gamma(shape=2.2), (_lib.LIK_GAMMA, 2.2)), (Beta(scale=3.5), (_lib.LIK_BETA, 3.5))]
    for lik, (kind, p0) in want:
        got = BroadcastingLikelihood(lik).mixture_args()
        assert got[0] == kind and got[1] == pytest.approx(p0, rel=1e-12), type(lik).__name__
    assert BroadcastingLikelihood(Poisson(binsize=0.8)).mixture_args()[2] == 0.8
    assert BroadcastingLikelihood(StudentT(1.3, 3.0)).mixture_args()[2] == 3.0
