"""-m gpu: the classification report of the predictive mixture on the device (csrc/classification.hip; dsdgp_mixture_classification,
dsdgp_model_classification, DGP_Base.classification_report) against tests/classification_reference.py.

Tolerances.  Per row, the probabilities, conf, l and brier: rtol 1e-10 / atol 1e-13 (the TOL of tests/test_gpu_evaluate.py); sums over n
rows n times the absolute part.  Every count entry exactly: each case of tests/classification_cases.py keeps the three margins of
classification_reference.margins above 1e-9 on every row (tests/test_classification_reference_cpu.py asserts it; asserted here again on
whatever reference a test builds itself), so no predicted class, bin or rank can differ under that tolerance, and no row is left out.
The all-classes-identical case is a constructed tie and states its own expectation.  The small models of tests/mixture_cases.py have
test rows far from every inducing point whose classes tie exactly; there the model-level tests hold the probabilities to the parent path
within the tolerance and the report to the reference evaluated on the device's own probabilities (ties broken by the stated rules),
and to the parent path's as well wherever its margins hold.

Shapes: tests/classification_cases.py lists them with what each is for.
DSDGP_CLASSIFICATION_PROFILE=<file> writes the measured worst error per case, device against reference and the two CPU versions of the
MultiClass probabilities against each other (profiles/classification_errors.md).

brier is the multi-class sum_c (pi_c - [c = y])^2: a binary (Bernoulli) problem gives 2 (p - t)^2."""
import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import classification_cases as CC
from tests import classification_reference as R
from tests.helpers import kern_spec, make_case
from tests.mixture_cases import NS, _case

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-13)
UNSUPPORTED, BAD_ARG = -4, -1
MULTICLASS, BERNOULLI, GAUSSIAN = 1, 2, 0
CANARY = -12345.25
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_CLASSIFICATION_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Classification report: measured errors (tests/test_gpu_classification.py)\n\n"
                "`probs`, `conf`, `l`, `brier`: the worst |device - reference| / (1e-13 + 1e-10 |reference|) over the case's rows (1 = at the\n"
                "tolerance); `sums`: the same for the floating-point entries of the accumulator with n x 1e-13; `counts`: entries that differ\n"
                "(held to 0).  `cpu`: the worst relative difference of the oracle's float64 MultiClass component probabilities to the\n"
                "independent evaluation on a subsample of (s, i) pairs.\n\n"
                "| case | probs | conf | l | brier | sums | counts | cpu |\n|---|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| %s | %.3g | %.3g | %.3g | %.3g | %.3g | %d | %s |\n" % r)


def _p(a):
    return C.c_void_p(a.data_ptr() if a is not None else 0)


def _nE(bins, Cn):
    return 4 + 3 * bins + Cn + Cn * Cn


def _cls(ctx, kind, mean, var, Y, bins, acc=None, accumulate=0, want_rows=True):
    """dsdgp_mixture_classification -> (acc (E + 1, ND) device tensor, probs (N, D) numpy or None, rows (N, ND, 4) numpy or None, return code).
    acc, rows_out and probs_out each carry one extra row filled with a canary that must survive."""
    S, N, D = mean.shape
    bern = kind == "bernoulli"
    Cn, ND = (2, D) if bern else (D, 1)
    E = _nE(bins, Cn) if 1 <= bins <= 32 else 1
    m, v, y = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(Y)
    with ctx.torch.cuda.stream(ctx.tstream):
        if acc is None:
            acc = ctx.empty(E + 1, ND)
            acc.fill_(CANARY)
        rows = ctx.empty(N + 1, ND, 4).fill_(CANARY) if want_rows else None
        probs = ctx.empty(N + 1, D).fill_(CANARY) if want_rows else None
    rc = ctx.lib.dsdgp_mixture_classification(ctx.handle, BERNOULLI if bern else MULTICLASS, _p(m), _p(v), _p(y), N, S, D, bins, _p(probs),
                                              _p(rows), _p(acc), accumulate)
    ctx.sync()
    if rc != 0:
        return acc, None, None, rc
    a = acc.cpu().numpy()
    assert np.all(a[E:] == CANARY), "dsdgp_mixture_classification wrote past acc"
    if not want_rows:
        return acc, None, None, rc
    r, p = rows.cpu().numpy(), probs.cpu().numpy()
    assert np.all(r[N:] == CANARY), "dsdgp_mixture_classification wrote past rows_out"
    assert np.all(p[N:] == CANARY), "dsdgp_mixture_classification wrote past probs_out"
    return acc, p[:N], r[:N], rc


def _ratio(got, want, atol=TOL["atol"]):
    return float(np.max(np.abs(got - want) / (atol + TOL["rtol"] * np.abs(want))))


def _check(name, ref, acc, probs, rows, bins, Cn, cpu=""):
    """device against reference (Cn classes: K, or 2 for Bernoulli): per-row values within TOL, count entries exactly, floating-point
    sums within n x atol"""
    assert min(float(m.min()) for m in ref["margins"]) > CC.MARGIN, "the reference's margins do not pin the counts"
    n = ref["rows"].shape[0]
    E = _nE(bins, Cn)
    assert ref["sums"].shape[0] == E, "the reference's accumulator does not have 4 + 3 B + C + C^2 entries"
    got = acc.cpu().numpy()[:E]
    cnt, val = R.count_rows(bins, Cn), R.value_rows(bins)
    fig = (name, _ratio(probs, ref["pbar"]), _ratio(rows[..., 1], ref["rows"][..., 1]), _ratio(rows[..., 2], ref["rows"][..., 2]),
           _ratio(rows[..., 3], ref["rows"][..., 3]), _ratio(got[val], ref["sums"][val], n * TOL["atol"]),
           int(np.sum(got[cnt] != ref["sums"][cnt])), cpu)
    print("%s: probs %.3g conf %.3g l %.3g brier %.3g sums %.3g (x tolerance), %d count entries differ %s" % fig)
    _ROWS.append(fig)
    assert np.all(np.isfinite(probs)) and np.all(np.isfinite(rows)) and np.all(np.isfinite(got))
    assert_allclose(probs, ref["pbar"], **TOL)
    assert np.array_equal(rows[..., 0], ref["rows"][..., 0])
    assert_allclose(rows[..., 1:], ref["rows"][..., 1:], **TOL)
    assert np.array_equal(got[cnt], ref["sums"][cnt])
    assert_allclose(got[val], ref["sums"][val], rtol=TOL["rtol"], atol=n * TOL["atol"])


@pytest.mark.parametrize("name", CC.NAMES)
def test_primitive_cases(ctx, name):
    ref = CC.reference(name)
    acc, probs, rows, rc = _cls(ctx, ref["kind"], ref["mean"], ref["var"], ref["Y"], ref["bins"])
    assert rc == 0, ctx.lib.dsdgp_last_error()
    cpu = ""
    if os.environ.get("DSDGP_CLASSIFICATION_PROFILE") and ref["kind"] == "multiclass":
        K = ref["mean"].shape[2]
        idx, want, how = R.independent_multiclass_probs(ref["mean"], ref["var"])
        mine = R.class_probs("multiclass", ref["mean"].reshape(1, -1, K)[:, idx], ref["var"].reshape(1, -1, K)[:, idx])[0]
        cpu = "%.3g (%d pairs, %s)" % (np.max(np.abs(mine - want) / np.abs(want)), len(idx), how)
    _check(name, ref, acc, probs, rows, ref["bins"], 2 if ref["kind"] == "bernoulli" else ref["mean"].shape[2], cpu)


def test_primitive_variances_at_and_below_the_clips_stay_finite(ctx):
    kind, bins, mean, var, Y = CC.clipped_variances()
    ref = CC.reference_of(kind, mean, var, Y, bins)
    acc, probs, rows, rc = _cls(ctx, kind, mean, var, Y, bins)
    assert rc == 0
    _check("clipped variances", ref, acc, probs, rows, bins, mean.shape[2])
    # Bernoulli: a zero variance is the plain probit of the mean
    _, b, bm, bv, bY = CC.inputs("bern_37_3_5")
    bv = bv.copy()
    bv[:, ::2] = 0.0
    ref = CC.reference_of("bernoulli", bm, bv, bY, b)
    acc, probs, rows, rc = _cls(ctx, "bernoulli", bm, bv, bY, b)
    assert rc == 0
    _check("zero variances, Bernoulli", ref, acc, probs, rows, b, 2)


def test_primitive_all_classes_identical(ctx):
    """mean and var equal across the classes: the K integrals see the same numbers, so a row's K probabilities are bit-equal (each 1/K up
    to the RobustMax floor and the quadrature); argmax takes the lowest class, and the label's rank counts the classes below it"""
    rng = np.random.RandomState(3)
    S, n, K, bins = 5, 9, 7, 10
    mean = np.repeat(rng.randn(S, n, 1), K, axis=2)
    var = np.repeat(rng.uniform(0.1, 1.0, size=(S, n, 1)), K, axis=2)
    Y = (np.arange(n) % K).astype(np.float64)[:, None]
    acc, probs, rows, rc = _cls(ctx, "multiclass", mean, var, Y, bins)
    assert rc == 0
    assert np.all(probs == probs[:, :1])
    assert_allclose(probs, R.mixture_probs("multiclass", mean, var), **TOL)
    assert np.array_equal(rows[:, 0, 0], np.zeros(n))
    got = acc.cpu().numpy()[:_nE(bins, K), 0]
    assert np.array_equal(got[4 + 3 * bins:4 + 3 * bins + K], np.bincount(Y[:, 0].astype(int), minlength=K))          # rank == label
    assert got[0] == np.sum(Y[:, 0] != 0) and got[3] == n
    conf = got[4 + 3 * bins + K:].reshape(K, K)
    assert np.array_equal(conf[:, 0], np.bincount(Y[:, 0].astype(int), minlength=K)) and conf[:, 1:].sum() == 0


def test_primitive_confident_and_wrong_rows(ctx):
    """pi_y a little above the floor eps / (K - 1): l is finite and the reference's"""
    kind, bins, mean, var, Y = CC.confident_and_wrong()
    ref = CC.reference_of(kind, mean, var, Y, bins)
    acc, probs, rows, rc = _cls(ctx, kind, mean, var, Y, bins)
    assert rc == 0
    _check("confident and wrong", ref, acc, probs, rows, bins, mean.shape[2])
    assert np.all(rows[:5, 0, 2] < np.log(2.0 * R.EPS / 2.0)) and np.all(rows[:5, 0, 2] > np.log(R.EPS / 2.0))
    assert acc.cpu().numpy()[0, 0] == 5.0


def test_primitive_bernoulli_targets(ctx):
    """targets -1 / 1 and 0 / 1 name the same classes: the same report, bit for bit; a p of exactly 0.5 predicts class 0"""
    ref = CC.reference("bern_37_3_5")
    a1, p1, r1, rc = _cls(ctx, "bernoulli", ref["mean"], ref["var"], ref["Y"], ref["bins"])
    assert rc == 0
    a2, p2, r2, rc = _cls(ctx, "bernoulli", ref["mean"], ref["var"], np.where(ref["Y"] == 1.0, 1.0, 0.0), ref["bins"])
    assert rc == 0
    assert np.array_equal(a1.cpu().numpy(), a2.cpu().numpy()) and np.array_equal(p1, p2) and np.array_equal(r1, r2)
    # mean 0: probit(0) = 0.5 (1 - 2e-3) + 1e-3 = 0.5 exactly
    z = np.zeros((2, 3, 1))
    acc, p, r, rc = _cls(ctx, "bernoulli", z, np.ones_like(z), np.array([[1.0], [-1.0], [0.0]]), 4)
    assert rc == 0 and np.all(p == 0.5)
    assert np.array_equal(r[:, 0, 0], np.zeros(3)) and np.all(r[:, 0, 1] == 0.5) and np.all(r[:, 0, 3] == 0.5)
    got = acc.cpu().numpy()[:_nE(4, 2), 0]
    assert got[0] == 1.0 and got[4 + 2] == 3.0 and np.array_equal(got[4 + 3 * 4:4 + 3 * 4 + 2], [2.0, 1.0])          # the label 1 ranks second
    assert np.array_equal(got[4 + 3 * 4 + 2:], [2.0, 0.0, 1.0, 0.0])


@pytest.mark.parametrize("name", ["mc_17_3_3", "mc_300_10_100", "mc_4099_5_5", "bern_37_3_5", "bern_4096_2_17"])
def test_primitive_accumulates_and_repeats_bitwise(ctx, name):
    ref = CC.reference(name)
    kind, mean, var, Y, bins = ref["kind"], ref["mean"], ref["var"], ref["Y"], ref["bins"]
    n = Y.shape[0]
    Cn = 2 if kind == "bernoulli" else mean.shape[2]
    E = _nE(bins, Cn)
    h = n // 2 + 1
    c = np.ascontiguousarray
    acc, _, _, rc = _cls(ctx, kind, c(mean[:, :h]), c(var[:, :h]), Y[:h], bins, want_rows=False)
    assert rc == 0
    acc, _, _, rc = _cls(ctx, kind, c(mean[:, h:]), c(var[:, h:]), Y[h:], bins, acc=acc, accumulate=1, want_rows=False)
    assert rc == 0
    got = acc.cpu().numpy()[:E]
    cnt, val = R.count_rows(bins, Cn), R.value_rows(bins)
    assert np.array_equal(got[cnt], ref["sums"][cnt])
    assert_allclose(got[val], ref["sums"][val], rtol=TOL["rtol"], atol=n * TOL["atol"])
    a1, p1, r1, _ = _cls(ctx, kind, mean, var, Y, bins)
    a2, p2, r2, _ = _cls(ctx, kind, mean, var, Y, bins)
    assert np.array_equal(a1.cpu().numpy(), a2.cpu().numpy()) and np.array_equal(p1, p2) and np.array_equal(r1, r2)
    # a row's probabilities do not depend on how many rows the call holds
    if kind == "multiclass":
        _, ph, _, _ = _cls(ctx, kind, c(mean[:, :h]), c(var[:, :h]), Y[:h], bins)
        assert np.array_equal(ph, p1[:h])


def test_primitive_works_without_the_optional_outputs(ctx):
    ref = CC.reference("mc_37_10_37")
    acc, _, _, rc = _cls(ctx, ref["kind"], ref["mean"], ref["var"], ref["Y"], ref["bins"], want_rows=False)
    assert rc == 0
    full, _, _, _ = _cls(ctx, ref["kind"], ref["mean"], ref["var"], ref["Y"], ref["bins"])
    assert np.array_equal(acc.cpu().numpy(), full.cpu().numpy())


def test_primitive_rejects_bad_arguments(ctx):
    _, _, mean, var, Y = CC.inputs("mc_17_3_3")
    err = ctx.lib.dsdgp_last_error
    who = b"dsdgp_mixture_classification"
    for bins in (0, 33, -5):
        assert _cls(ctx, "multiclass", mean, var, Y, bins)[3] == BAD_ARG and who in err() and b"bins" in err()
    m1 = np.zeros((2, 4, 1))
    assert _cls(ctx, "multiclass", m1, np.ones_like(m1), np.zeros((4, 1)), 10)[3] == UNSUPPORTED and who in err() and b"K=1" in err()
    m33 = np.zeros((1, 4, 33))
    assert _cls(ctx, "multiclass", m33, np.ones_like(m33), np.zeros((4, 1)), 10)[3] == UNSUPPORTED and who in err() and b"K=33" in err()
    m, v, y = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(Y)
    acc = ctx.empty(_nE(10, 3), 1)
    S, N, K = mean.shape
    for kind in (GAUSSIAN, 3, 7, 99):
        rc = ctx.lib.dsdgp_mixture_classification(ctx.handle, kind, _p(m), _p(v), _p(y), N, S, K, 10, None, None, _p(acc), 0)
        assert rc == UNSUPPORTED and who in err() and b"no classes" in err()
    assert ctx.lib.dsdgp_mixture_classification(ctx.handle, MULTICLASS, _p(m), _p(v), _p(y), 0, S, K, 10, None, None, _p(acc), 0) == BAD_ARG
    assert ctx.lib.dsdgp_mixture_classification(ctx.handle, MULTICLASS, _p(m), _p(v), _p(y), N, 0, K, 10, None, None, _p(acc), 0) == BAD_ARG
    assert ctx.lib.dsdgp_mixture_classification(ctx.handle, MULTICLASS, _p(m), _p(v), _p(y), N, S, K, 10, None, None, None, 0) == BAD_ARG
    ctx.sync()


# ---------------------------------------------------------------- model level
_refs = {}


def _kind(name):
    return "bernoulli" if name == "bernoulli" else "multiclass"


def _forward(name, S):
    """the parent path: predict_y on all rows at once under the case's draws — computed once per (model, S)"""
    if (name, S) not in _refs:
        model, Xs, Ys, zs = _case(name)
        Fm, Fv = model._build_predict(Xs, S=S, zs=[z[:S] for z in zs])
        P, _ = model.likelihood.predict_mean_and_var(Fm, Fv)
        _refs[name, S] = (Fm, Fv, P.mean(0))
    return _refs[name, S]


def _same_report(out, want):
    """every count-derived entry exactly, the floating-point ones within TOL"""
    assert out["error_rate"] == want["error_rate"]
    assert np.array_equal(out["confusion"], want["confusion"]) and out["confusion"].dtype == np.int64
    assert np.array_equal(out["top_k_accuracy"], want["top_k_accuracy"])
    assert np.array_equal(out["reliability"]["count"], want["reliability"]["count"])
    assert_allclose(out["reliability"]["confidence"], want["reliability"]["confidence"], equal_nan=True, **TOL)
    assert np.array_equal(out["reliability"]["accuracy"], want["reliability"]["accuracy"], equal_nan=True)
    assert_allclose(out["ece"], want["ece"], **TOL)
    assert_allclose(out["mce"], want["mce"], **TOL)
    for q in ("recall", "precision", "support"):
        assert np.array_equal(out["per_class"][q], want["per_class"][q], equal_nan=True)
    for k in ("log_density", "brier", "error_rate_per_output", "log_density_per_output", "brier_per_output", "ece_per_output"):
        assert (k in out) == (k in want)
        if k in want:
            assert_allclose(out[k], want[k], **TOL)


def _check_report(out, kind, pbar, Ys, bins):
    """a report against the reference built on the parent path's mixture probabilities `pbar`: the values within TOL; the predicted
    class on every row whose margins exceed 1e-9, and every count where that holds for all rows (printed where it does not)"""
    top, binm, lab = R.margins(kind, pbar, Ys, bins)
    ok = (top > CC.MARGIN) & (binm > CC.MARGIN) & (lab > CC.MARGIN)
    pinned = bool(ok.all())
    if not pinned:
        print("margins at or below 1e-9 (item, top two, conf B to an integer, pi_c to pi_y):",
              [(tuple(i), top[tuple(i)], binm[tuple(i)], lab[tuple(i)]) for i in np.argwhere(~ok)])
    n = Ys.shape[0]
    Cn = 2 if kind == "bernoulli" else pbar.shape[1]
    want = R.scores(R.sums(kind, pbar, Ys, bins), bins, Cn)
    assert out["n"] == n
    if "probs" in out:
        assert_allclose(out["probs"], pbar, **TOL)
        ref_rows = R.rows(kind, pbar, Ys, bins)
        assert_allclose(out["rows"][..., 1:], ref_rows[..., 1:], **TOL)
        assert np.array_equal(out["rows"][..., 0][ok], ref_rows[..., 0][ok])
    for k in ("log_density", "brier"):
        assert_allclose(out[k], want[k], **TOL)
    if pinned:
        _same_report(out, want)
    if "probs" in out:
        # the small models have rows far from every inducing point whose classes tie (a Bernoulli p of exactly 0.5, K equal
        # probabilities): from the device's own probabilities the report is pinned whatever the margins, ties by the stated rules
        _same_report(out, R.scores(R.sums(kind, out["probs"], Ys, bins), bins, Cn))
        assert np.array_equal(out["rows"][..., 0], R.rows(kind, out["probs"], Ys, bins)[..., 0])
    return pinned


@pytest.mark.parametrize("S", [1, 3, 37])
@pytest.mark.parametrize("batch_size", [16, 37, 1000])
@pytest.mark.parametrize("name", ["bernoulli", "multiclass"])
def test_model_matches_the_parent_path(name, batch_size, S):
    model, Xs, Ys, zs = _case(name)
    _, _, pbar = _forward(name, S)
    out = model.classification_report(Xs, Ys, S, batch_size=batch_size, zs=[q[:S] for q in zs], return_rows=True)
    D = pbar.shape[1]
    assert out["probs"].shape == (NS, D) and out["rows"].shape == (NS, D if name == "bernoulli" else 1, 4)
    assert_allclose(out["probs"], pbar, **TOL)
    _check_report(out, _kind(name), pbar, Ys, 10)
    if name == "bernoulli":
        assert out["confusion"].shape == (D, 2, 2) and out["reliability"]["count"].shape == (D, 10)


@pytest.mark.parametrize("name", ["bernoulli", "multiclass"])
def test_model_agrees_with_evaluate(name):
    """error_rate (MultiClass) and log_density are evaluate's, from the same draws"""
    model, Xs, Ys, zs = _case(name)
    S = 3
    z = [q[:S] for q in zs]
    _, _, pbar = _forward(name, S)
    out = model.classification_report(Xs, Ys, S, batch_size=16, zs=z, bins=7)
    ev = model.evaluate(Xs, Ys, S, batch_size=16, zs=z)
    assert_allclose(out["log_density"], ev["log_density"], **TOL)
    if name == "multiclass":
        assert "error_rate" in ev
        if min(float(m.min()) for m in R.margins("multiclass", pbar, Ys, 7)) > CC.MARGIN:      # (no tie that the two routes may break differently)
            assert out["error_rate"] == ev["error_rate"]
        else:
            print("a margin at or below 1e-9: the error counts are not compared")
    assert "rows" not in out and "probs" not in out


@pytest.mark.parametrize("name", ["bernoulli", "multiclass"])
def test_model_takes_device_tensors_and_broadcast_draws(name):
    model, Xs, Ys, zs = _case(name)
    ctx = model.engine().ctx
    S = 3
    zb = [zs[0][:S, :1], zs[1][:1]]                      # one draw shared by all rows / by all samples
    Fm, Fv = model._build_predict(Xs, S=S, zs=zb)
    pbar = model.likelihood.predict_mean_and_var(Fm, Fv)[0].mean(0)
    zd = [ctx.to_device(z) for z in zb]
    out = model.classification_report(ctx.to_device(Xs), ctx.to_device(Ys), S, batch_size=16, zs=zd, return_rows=True)
    _check_report(out, _kind(name), pbar, Ys, 10)


def test_model_device_draws_use_one_seed_per_batch():
    """zs = None: batch k of a call draws under the k-th _draw_seed() after the call's start (world = 1: seed + k + 1);
    predict_y on the same rows under the same seed is the parent path"""
    model, Xs, Ys, _ = _case("multiclass")
    S, bs = 3, 16
    s0 = model._seed
    out = model.classification_report(Xs, Ys, S, batch_size=bs, return_rows=True)
    assert model._seed == s0 + 3
    P = []
    for k, a in enumerate(range(0, NS, bs)):
        model._seed = s0 + k
        P.append(model.predict_y(Xs[a:a + bs], S)[0].mean(0))
    model._seed = s0 + 3
    _check_report(out, "multiclass", np.concatenate(P, 0), Ys, 10)


def test_model_refusals_reach_the_caller():
    from doubly_stochastic_dgp import _lib
    gauss, Xs, Ys, _ = _case("rbf")
    with pytest.raises(NotImplementedError):
        gauss.classification_report(Xs, Ys[:, :1], 3)
    eng = gauss.engine()
    ctx = eng.ctx
    Xd, Yd, acc = ctx.to_device(Xs), ctx.to_device(Ys), ctx.empty(_nE(10, 2), 2)
    rc = ctx.lib.dsdgp_model_classification(eng.model, _p(Xd), _p(Yd), NS, 3, None, None, C.c_uint64(1), 10, None, None, _p(acc), 0)
    assert rc == UNSUPPORTED and b"dsdgp_model_classification" in ctx.lib.dsdgp_last_error() and b"no classes" in ctx.lib.dsdgp_last_error()
    # a model carrying quadrature sample weights (DGP_Quad sets them) is not an unweighted mixture
    model, Xs, Ys, zs = _case("multiclass")
    eng = model.engine()
    eng.set_sample_weights(eng.ctx.to_device(np.full(3, 1.0 / 3.0)))
    try:
        with pytest.raises(_lib.DsdgpError, match="-4"):
            model.classification_report(Xs, Ys, 3)
        assert b"sample weights" in ctx.lib.dsdgp_last_error() and b"dsdgp_model_classification" in ctx.lib.dsdgp_last_error()
    finally:
        eng.set_sample_weights(None)
    Xd, Yd, acc = ctx.to_device(Xs), ctx.to_device(Ys), ctx.empty(_nE(10, 3), 1)
    rc = ctx.lib.dsdgp_model_classification(eng.model, _p(Xd), _p(Yd), NS, 3, None, None, C.c_uint64(1), 40, None, None, _p(acc), 0)
    assert rc == BAD_ARG and b"bins = 40" in ctx.lib.dsdgp_last_error()
    ctx.sync()
    assert np.isfinite(model.classification_report(Xs, Ys, 3)["ece"])


def test_model_equals_the_primitive_bit_for_bit():
    from doubly_stochastic_dgp.dgp import classification_scores
    for name in ("bernoulli", "multiclass"):
        model, Xs, Ys, zs = _case(name)
        S = 3
        Fm, Fv, _ = _forward(name, S)
        out = model.classification_report(Xs, Ys, S, zs=[q[:S] for q in zs], bins=5, return_rows=True)
        acc, probs, rows = model.likelihood.mixture_classification(Fm, Fv, Ys, bins=5, rows=True)
        want = classification_scores(acc, 5, 2 if name == "bernoulli" else 3)
        assert np.array_equal(probs, out["probs"]) and np.array_equal(rows, out["rows"])
        assert want["ece"] == out["ece"] and want["brier"] == out["brier"] and np.array_equal(want["confusion"], out["confusion"])


def test_report_between_training_steps_leaves_their_bits():
    """two models take the same two optimiser steps; one of them reports on held-out rows (another row count, another S) in between"""
    rng = np.random.RandomState(9)
    N, D, M, S, K = 40, 2, 16, 3, 3
    X, Y = rng.randn(N, D), rng.randint(0, K, size=(N, 1)).astype(np.float64)
    Z = X[:M] + 0.01 * rng.randn(M, D)
    specs = [kern_spec("rbf", D, 1.2, 0.9)] * 2
    Xs, Ys = rng.randn(NS, D), rng.randint(0, K, size=(NS, 1)).astype(np.float64)
    zs = [rng.randn(S, N, 2), rng.randn(S, N, K)]
    thetas, elbos = [], []
    for between in (False, True):
        _, _, model = make_case(X, Y, Z, specs, lik_var=0.1, S=S, seed=3, num_classes=K)
        eng = model.engine()
        eng._ensure(N, 5)
        e = [model.train_step(X=X, Y=Y, zs=zs, sync=True)]
        if between:
            out = model.classification_report(Xs, Ys, 5, batch_size=16)
            assert np.isfinite(out["ece"]) and out["confusion"].sum() == NS
        e.append(model.train_step(X=X, Y=Y, zs=zs, sync=True))
        eng.ctx.sync()
        thetas.append(eng.theta.cpu().numpy().copy())
        elbos.append(e)
    assert elbos[0] == elbos[1]
    assert np.array_equal(thetas[0].view(np.uint64), thetas[1].view(np.uint64))
