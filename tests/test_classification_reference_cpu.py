"""The CPU reference of tests/test_gpu_classification.py (tests/classification_reference.py) and its case table
(tests/classification_cases.py) pinned on their own, without a GPU: every case keeps the three margins that pin the counts; the
identities a classification report obeys; a perfectly calibrated table has ece = 0; log_density is evaluate's; a second, independent
evaluation of the MultiClass probabilities agrees with the oracle's — and the host side of the feature that needs no device: the two
C-ABI entries are declared with the argument counts of include/dsdgp.h, the scores are formed from the accumulator as documented, and
every argument DGP_Base.classification_report refuses is refused before a device is looked for.

Two kinds of test, then.  Those above the "host side" rule (margins, identities, log density, the two CPU versions, ties) check only
tests/classification_reference.py and the case table: they guard the yardstick the GPU tests measure against, import nothing of the
package's new code and pass with or without it.  test_a_perfectly_calibrated_table_has_zero_ece and
test_package_scores_equal_the_reference_scores (dgp.classification_scores) and every test below the rule call the package: without the
feature they fail on the missing name, symbol or method."""
import ctypes
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import classification_cases as CC
from tests import classification_reference as R
from tests import evaluate_reference as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", CC.NAMES)
def test_every_case_keeps_its_margins(name):
    r = CC.reference(name)
    worst = [float(m.min()) for m in r["margins"]]
    print(name, "smallest margins (top two, conf B to an integer, pi_c to pi_y):", worst)
    assert min(worst) > CC.MARGIN, (name, worst)
    assert np.all(np.isfinite(r["rows"]))


@pytest.mark.parametrize("make", [CC.clipped_variances, CC.confident_and_wrong])
def test_the_constructed_cases_keep_their_margins_too(make):
    kind, bins, mean, var, Y = make()
    r = CC.reference_of(kind, mean, var, Y, bins)
    assert min(float(m.min()) for m in r["margins"]) > CC.MARGIN and np.all(np.isfinite(r["rows"]))
    if make is CC.confident_and_wrong:
        K = mean.shape[2]
        piy = np.exp(r["rows"][:5, 0, 2])
        assert np.all(piy > R.EPS / (K - 1)) and np.all(piy < 2.0 * R.EPS / (K - 1))          # near the floor eps / (K - 1), above it
        assert np.array_equal(r["rows"][:, 0, 0], np.zeros(6)) and r["sums"][0, 0] == 5.0


@pytest.mark.parametrize("name", ["mc_17_3_3", "mc_37_10_37", "mc_64_32_2", "mc_4099_5_5", "bern_37_3_5", "bern_4096_2_3"])
def test_report_identities(name):
    r = CC.reference(name)
    s, B = r["sums"], r["bins"]
    kind = r["kind"]
    C = 2 if kind == "bernoulli" else r["mean"].shape[2]
    n = r["Y"].shape[0]
    ND = s.shape[1]
    assert np.array_equal(s[3], np.full(ND, n))
    assert np.array_equal(s[4:4 + B].sum(0), s[3])                                      # bin counts
    assert np.array_equal(s[4 + 3 * B:4 + 3 * B + C].sum(0), s[3])                      # rank histogram
    conf = s[4 + 3 * B + C:].reshape(C, C, ND)
    assert np.array_equal(conf.sum((0, 1)), s[3])
    assert np.array_equal(np.einsum("ttd->d", conf), s[3] - s[0])                       # trace = n - errors
    assert np.array_equal(s[4 + 2 * B:4 + 3 * B].sum(0), s[3] - s[0])                   # correct rows over the bins
    assert np.array_equal(s[4 + 3 * B], s[3] - s[0])                                    # rank 0 <=> predicted (no ties in the table)
    assert_allclose(s[4 + B:4 + 2 * B].sum(0), r["rows"][..., 1].sum(0), rtol=1e-13)
    assert np.array_equal(s[R.count_rows(B, C)], np.rint(s[R.count_rows(B, C)]))
    out = R.scores(s, B, C)
    assert out["top_k_accuracy"][-1] == 1.0 and np.all(np.diff(out["top_k_accuracy"]) >= 0.0)
    assert out["top_k_accuracy"][0] == (s[3] - s[0]).sum() / s[3].sum() and out["error_rate"] == s[0].sum() / s[3].sum()
    assert 0.0 <= out["ece"] <= out["mce"] <= 1.0
    # brier: the multi-class definition; a binary problem gives 2 (p - t)^2
    if kind == "bernoulli":
        t = (r["Y"] == 1.0).astype(np.float64)
        assert_allclose(r["rows"][..., 3], 2.0 * (r["pbar"] - t) ** 2, rtol=1e-12, atol=1e-300)


def test_a_perfectly_calibrated_table_has_zero_ece():
    """constructed sums: in every non-empty bin the mean confidence equals the accuracy exactly (dyadic numbers)"""
    B, C = 4, 2
    s = np.zeros((4 + 3 * B + C + C * C, 1))
    s[3] = 24
    s[4 + 2], s[4 + B + 2], s[4 + 2 * B + 2] = 16, 16 * 0.625, 10         # bin [0.5, 0.75): confidence 0.625, 10 of 16 right
    s[4 + 3], s[4 + B + 3], s[4 + 2 * B + 3] = 8, 8 * 0.875, 7            # bin [0.75, 1]: confidence 0.875, 7 of 8 right
    s[0] = 24 - 17
    s[4 + 3 * B], s[4 + 3 * B + 1] = 17, 7
    s[4 + 3 * B + C:, 0] = [9, 3, 4, 8]
    from doubly_stochastic_dgp.dgp import classification_scores
    for out in (R.scores(s, B, C), classification_scores(s, B, C)):
        assert out["ece"] == 0.0 and out["mce"] == 0.0
        assert np.array_equal(out["reliability"]["count"], [0, 0, 16, 8])
        assert np.all(np.isnan(out["reliability"]["confidence"][:2])) and np.all(np.isnan(out["reliability"]["accuracy"][:2]))
        assert np.array_equal(out["reliability"]["confidence"][2:], [0.625, 0.875])
        assert np.array_equal(out["reliability"]["accuracy"][2:], [0.625, 0.875])
        assert np.array_equal(out["reliability"]["edges"], [0.0, 0.25, 0.5, 0.75, 1.0])
        assert out["error_rate"] == 7 / 24 and np.array_equal(out["top_k_accuracy"], [17 / 24, 1.0])
        assert out["confusion"].dtype == np.int64 and np.array_equal(out["confusion"], [[9, 3], [4, 8]])
        assert np.array_equal(out["per_class"]["recall"], [9 / 12, 8 / 12]) and np.array_equal(out["per_class"]["support"], [12, 12])
        assert np.array_equal(out["per_class"]["precision"], [9 / 13, 8 / 11])
    # a miscalibrated bin shows: 16 rows of confidence 0.625 of which 12 are right
    s[4 + 2 * B + 2] = 12
    for out in (R.scores(s, B, C), classification_scores(s, B, C)):
        assert out["ece"] == 16 / 24 * 0.125 and out["mce"] == 0.125


@pytest.mark.parametrize("name", ["mc_37_10_37", "bern_4096_2_3", "bern_37_3_5"])
def test_package_scores_equal_the_reference_scores(name):
    from doubly_stochastic_dgp.dgp import classification_scores
    r = CC.reference(name)
    C = 2 if r["kind"] == "bernoulli" else r["mean"].shape[2]
    want, got = R.scores(r["sums"], r["bins"], C), classification_scores(r["sums"], r["bins"], C)
    assert want.keys() == got.keys()
    for k in want:
        if isinstance(want[k], dict):
            assert want[k].keys() == got[k].keys()
            for q in want[k]:
                assert np.shape(got[k][q]) == np.shape(want[k][q]), (k, q)
                assert_allclose(got[k][q], want[k][q], rtol=1e-13, atol=1e-15, equal_nan=True)
        else:
            assert np.shape(got[k]) == np.shape(want[k]), k
            assert_allclose(got[k], want[k], rtol=1e-13, atol=1e-15)
    D = r["sums"].shape[1]
    if D > 1:
        assert got["confusion"].shape == (D, 2, 2) and got["reliability"]["confidence"].shape == (D, r["bins"])
        assert got["ece_per_output"].shape == (D,)


def test_log_density_is_evaluates():
    """l = log of the averaged probability of the label = logsumexp_s log p_s(y) - log S, what evaluate_reference sums for MultiClass"""
    r = CC.reference("mc_37_10_37")
    P = R.class_probs("multiclass", r["mean"], r["var"])
    y = r["Y"][:, 0].astype(int)
    logp = np.log(P[:, np.arange(len(y)), y])[..., None]
    erows = ER.mixture_rows(logp, P, P - P ** 2)
    es = ER.multiclass_sums(erows, r["Y"])
    assert_allclose(r["sums"][1, 0], es[1, 0], rtol=1e-13)
    assert r["sums"][0, 0] == es[0, 0] and r["sums"][3, 0] == es[2, 0]
    assert_allclose(r["rows"][:, 0, 2], erows[:, 0, 2], rtol=1e-13, atol=1e-15)


_WORST = {}


@pytest.mark.parametrize("name", ["mc_1_2_1", "mc_17_3_3", "mc_37_10_37", "mc_64_32_2", "mc_300_10_100", "mc_4099_5_5"])
def test_two_cpu_versions_of_the_probabilities_agree(name):
    """the oracle's float64 component probabilities against an independent evaluation (30-digit mpmath where installed) on a subsample
    of the (s, i) pairs: the difference is the float64 version's own error, far inside the rtol 1e-10 the device is held to"""
    r = CC.reference(name)
    K = r["mean"].shape[2]
    idx, want, how = R.independent_multiclass_probs(r["mean"], r["var"])
    got = R.class_probs("multiclass", r["mean"].reshape(1, -1, K)[:, idx], r["var"].reshape(1, -1, K)[:, idx])[0]
    worst = float(np.max(np.abs(got - want) / np.abs(want)))
    _WORST[name] = worst
    print(f"{name}: {len(idx)} (s, i) pairs against {how}: worst relative difference {worst:.3g}")
    assert worst < 1e-12, (name, worst)


def test_the_reordered_float64_version_agrees_as_well():
    r = CC.reference("mc_17_3_3")
    P = R.class_probs("multiclass", r["mean"], r["var"]).reshape(-1, 3)
    m2, v2 = r["mean"].reshape(-1, 3), r["var"].reshape(-1, 3)
    alt = np.array([R._one_multiclass_reordered(m2[i], v2[i]) for i in range(len(P))])
    assert_allclose(alt, P, rtol=1e-12)


def test_margins_tell_a_tie():
    pbar = np.array([[0.2, 0.5, 0.3], [0.4, 0.4, 0.2], [0.25, 0.5, 0.25]])
    Y = np.array([[1.0], [2.0], [0.0]])
    top, binm, lab = R.margins("multiclass", pbar, Y, 10)
    assert_allclose(top[:, 0], [0.2, 0.0, 0.25], atol=1e-15)
    assert_allclose(binm[:, 0], [0.0, 0.0, 0.0], atol=1e-15)          # conf B = 5, 4, 5
    assert_allclose(lab[:, 0], [0.2, 0.2, 0.0], atol=1e-15)
    v = R.item_values("multiclass", pbar, Y, 10)
    assert np.array_equal(v["pred"][:, 0], [1, 0, 1]) and np.array_equal(v["rank"][:, 0], [0, 2, 1])          # ties: the lower class first
    assert np.array_equal(v["bin"][:, 0], [5, 4, 5])
    # conf = 1 lands in the last bin, a Bernoulli p of exactly 0.5 predicts class 0
    assert R.item_values("multiclass", np.array([[1.0, 0.0]]), np.array([[0.0]]), 10)["bin"][0, 0] == 9
    v = R.item_values("bernoulli", np.array([[0.5]]), np.array([[1.0]]), 4)
    assert v["pred"][0, 0] == 0 and v["rank"][0, 0] == 1 and v["bin"][0, 0] == 2


# ---------------------------------------------------------------- the host side that needs no device
def _header_arg_count(name):
    text = open(os.path.join(ROOT, "include", "dsdgp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/dsdgp.h"
    return len(m.group(1).split(","))


@pytest.mark.parametrize("name,count", [("dsdgp_mixture_classification", 13), ("dsdgp_model_classification", 13)])
def test_binding_declares_the_new_entry_points(name, count):
    from doubly_stochastic_dgp import _lib
    assert name in _lib.EXPORTED_SYMBOLS
    res, args = _lib._PROTOS[name]
    assert res is ctypes.c_int and len(args) == count == _header_arg_count(name)
    if os.path.exists(_lib.lib_path()):          # the built library exports it (dlopen needs no GPU)
        assert hasattr(ctypes.CDLL(_lib.lib_path()), name)
    assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _models():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Bernoulli, Gaussian, MultiClass
    rng = np.random.RandomState(0)
    X = rng.randn(20, 2)
    gauss = DGP(X, X[:, :1], X[:5], [RBF(2), RBF(2)], Gaussian())
    bern = DGP(X, np.sign(X[:, :2]), X[:5], [RBF(2), RBF(2)], Bernoulli())
    labels = rng.randint(0, 3, size=(20, 1)).astype(np.float64)
    mc = DGP(X, labels, X[:5], [RBF(2), RBF(2)], MultiClass(3), num_outputs=3)
    return X, labels, gauss, bern, mc


def test_host_refusals_come_before_the_device():
    """every refused argument raises its own error whether or not a GPU is present: nothing below touches the engine"""
    X, labels, gauss, bern, mc = _models()
    with pytest.raises(NotImplementedError, match="no classes"):
        gauss.classification_report(X, X[:, :1], 3)
    with pytest.raises(NotImplementedError):
        gauss.likelihood.mixture_classification(np.zeros((2, 3, 1)), np.ones((2, 3, 1)), np.zeros((3, 1)))
    Yb = np.sign(X[:, :2])
    for model, Y in ((mc, labels), (bern, Yb)):
        for bins in (0, 33, -1):
            with pytest.raises(ValueError, match="bins"):
                model.classification_report(X, Y, 3, bins=bins)
        for kw in (dict(batch_size=0), dict(zs=[None]), dict(zs=[np.zeros((3, 2)), None])):
            with pytest.raises(ValueError):
                model.classification_report(X, Y, 3, **kw)
        for S in (0, -2):
            with pytest.raises(ValueError):
                model.classification_report(X, Y, S)
        with pytest.raises(ValueError, match="shape"):
            model.classification_report(X, Y[:-1], 3)
        with pytest.raises(ValueError):
            model.classification_report(X[:0], Y[:0], 3)
        with pytest.raises(ValueError):
            model.classification_report(X[:, 0], Y, 3)
    with pytest.raises(ValueError, match="shape"):
        mc.classification_report(X, np.zeros((20, 3)), 3)          # one-hot instead of labels
    with pytest.raises(ValueError, match="shape"):
        bern.classification_report(X, Yb[:, :1], 3)                # one output of two
    for bad in (np.full((20, 1), 3.0), np.full((20, 1), -1.0), np.full((20, 1), 0.5), np.full((20, 1), np.nan)):
        with pytest.raises(ValueError, match="labels"):            # what check_targets raises
            mc.classification_report(X, bad, 3)
    with pytest.raises(ValueError, match="bins"):
        mc.likelihood.mixture_classification(np.zeros((2, 20, 3)), np.ones((2, 20, 3)), labels, bins=33)
    with pytest.raises(ValueError, match="shape"):
        mc.likelihood.mixture_classification(np.zeros((2, 19, 3)), np.ones((2, 19, 3)), labels)


def test_valid_arguments_reach_the_device_or_its_absence():
    """with valid arguments the call goes on to the engine: without a GPU that is the library's "no CPU fallback" error"""
    import torch
    from doubly_stochastic_dgp import _lib
    X, labels, gauss, bern, mc = _models()
    calls = [lambda: mc.classification_report(X, labels, 3)["confusion"], lambda: bern.classification_report(X, np.sign(X[:, :2]), 3)["confusion"]]
    for call, shape in zip(calls, [(3, 3), (2, 2, 2)]):
        if torch.cuda.is_available():
            assert call().shape == shape
        else:
            with pytest.raises(_lib.DsdgpError, match="no CPU fallback"):
                call()
