"""tests/likelihood_reference.py held to its own bars (no GPU): the two float64 comparators against the 40-digit truth and against each
other, the truth's analytic derivatives against central differences of the truth's own values, the torch-autograd gradient of the oracle's
variational_expectations against the truth, and the case table against the list of edges it promises."""
import numpy as np
import pytest

from oracle import dgp_oracle as O
from tests import likelihood_reference as LR
from tests.factor_reference import device_bar
from tests.likelihood_cases import (BETA_SCALES, BETA_TARGETS, ELEMENT_CASES, GAMMA_SHAPES, LAYOUT_SHAPES, MULTICLASS_CASES,
                                    POISSON_COUNTS, SMALL_V, STUDENT_NU, element_case)

CPU_ELEMENT = [c for c in ELEMENT_CASES if c["name"].endswith(("-ordinary", "-small-v")) or c["name"] in
               ("gamma-shape7.9", "gamma-shape8.1", "beta-scale0.05", "poisson-counts-binsize1", "student_t-nu0.5-scale0.001",
                "bernoulli-large-mean-pm1")]
CPU_MULTI = [c for c in MULTICLASS_CASES if c["name"] in ("mc-ordinary-K2-R1", "mc-ordinary-K3-R15", "mc-ordinary-K10-R16", "mc-clips-K3-R17",
                                                          "mc-clips-mixed-K3-R17", "mc-separated-K3-R4")]


def _agree(T, name):
    """each comparator within the bar the OTHER one alone would set: neither inflates the device's bar by an error of its own"""
    for q in T["numpy"]:
        a, b = T["numpy"][q], T["torch"][q]
        assert np.isfinite(a) and np.isfinite(b), (name, q, a, b)
        assert max(a, b) <= device_bar(min(a, b), 0), (name, q, a, b)
        assert T["bars"][q] == max(1.0, 8.0 * max(a, b))


@pytest.mark.parametrize("case", CPU_ELEMENT, ids=lambda c: c["name"])
def test_comparators_against_the_truth(case):
    T = LR.element_truth(case)
    assert set(T["truth"]) == set(LR.ELEMENT_QUANTITIES)
    _agree(T, case["name"])
    if case["kind"] not in LR.HAS_PARAM:
        assert np.all(T["truth"]["dp0"][0] == 0)


@pytest.mark.parametrize("case", CPU_MULTI, ids=lambda c: c["name"])
def test_multiclass_comparators_against_the_truth(case):
    T = LR.multiclass_truth(case)
    _agree(T, case["name"])
    S, N, K = case["mean"].shape
    var = case["var"].reshape(S * N, K)
    is_y = np.arange(K)[None, :] == T["labels"][:, None]
    gated = np.where(is_y, var <= 0.5e-10, var <= 1e-10)
    dv = T["truth"]["dvar"][0]
    assert np.all(dv[gated & T["masks"]["dvar"]] == 0), "a clipped variance passes no gradient"
    p = T["truth"]["p"][0]
    assert np.all((p > 0) & (p < 1))


def _sub(case, idx):
    return case["mu"][idx], case["v"][idx], case["y"][idx]


@pytest.mark.parametrize("name", ["bernoulli-ordinary", "student_t-ordinary", "beta-ordinary", "gamma-ordinary", "poisson-ordinary",
                                  "exponential-ordinary", "gaussian-ordinary", "beta-small-v", "student_t-small-v", "bernoulli-small-v",
                                  "gamma-shape8.1", "beta-scale0.05"])
def test_truth_derivatives_against_central_differences(name):
    """d ve / d(mu, v, p0) of the rule in 40 digits against (ve(x + h) - ve(x - h)) / (2 h) in 40 digits, h = 1e-6 of the argument (the
    perturbed float64 arguments are exact inputs; the truncation error is ~ 1e-12 of the third derivative's scale): 1e-8 of the
    derivative's own scale.  A wrong sign, factor or chain rule is an error of order one."""
    case = element_case(name)
    idx = np.arange(0, case["mu"].size, 7)
    idx = idx[case["v"][idx] != 0.0]
    mu, v, y = _sub(case, idx)
    kind, p0, p1 = case["kind"], case["p0"], case["p1"]
    tr = LR.elementwise(LR.MP, kind, mu, v, y, p0, p1, which=("dmu", "dv", "dp0"))

    def ve(mu_, v_, p0_):
        return LR.elementwise(LR.MPRAW, kind, mu_, v_, y, p0_, p1, which=("ve",))["ve"][0]

    def quotient(up, dn, xu, xd):      # the difference quotient formed in mpmath (a v of 1e-30 moves ve by 1e-36), then rounded
        import mpmath
        with mpmath.workdps(LR.MP.DPS):
            return LR.MP.out((up - dn) / (LR.MP.arr(np.broadcast_to(xu, mu.shape)) - LR.MP.arr(np.broadcast_to(xd, mu.shape))))

    hm = 1e-6 * np.maximum(1.0, np.abs(mu))
    fd = {"dmu": quotient(ve(mu + hm, v, p0), ve(mu - hm, v, p0), mu + hm, mu - hm)}
    vp, vm = v * (1.0 + 1e-6), v * (1.0 - 1e-6)
    fd["dv"] = quotient(ve(mu, vp, p0), ve(mu, vm, p0), vp, vm)
    if kind in LR.HAS_PARAM:
        pp, pm = p0 * (1.0 + 1e-6), p0 * (1.0 - 1e-6)
        fd["dp0"] = quotient(ve(mu, v, pp), ve(mu, v, pm), pp, pm)
    for q, d in fd.items():
        val, sc = tr[q]
        assert np.all(np.abs(d - val) <= 1e-8 * np.maximum(sc, np.abs(val))), (name, q, float(np.max(np.abs(d - val) / np.maximum(sc, np.abs(val)))))


def test_multiclass_truth_derivatives_against_central_differences():
    case = next(c for c in MULTICLASS_CASES if c["name"] == "mc-ordinary-K3-R15")
    mean, var, lab = case["mean"][0], case["var"][0], case["labels"].reshape(-1)
    tr = LR.multiclass(LR.MP, mean, var, lab, w=0.75)
    for which, arr in (("dmean", mean), ("dvar", var)):
        for k in range(3):
            h = np.zeros_like(arr)
            h[:, k] = 1e-6
            up, dn = arr + h, arr - h
            a = (up, var) if which == "dmean" else (mean, up)
            b = (dn, var) if which == "dmean" else (mean, dn)
            d = (LR.multiclass(LR.MP, *a, lab)["ve"][0] - LR.multiclass(LR.MP, *b, lab)["ve"][0]) / (
                np.asarray(up[:, k], np.longdouble) - np.asarray(dn[:, k], np.longdouble))
            val, sc = tr[which][0][:, k], tr[which][1][:, k]
            assert np.all(np.abs(-0.75 * d - val) <= 1e-8 * np.maximum(sc, np.abs(val))), (which, k)


ORACLE = {"gaussian": lambda p0, p1: O.Gaussian(p0), "bernoulli": lambda p0, p1: O.Bernoulli(), "poisson": lambda p0, p1: O.Poisson(p1),
          "exponential": lambda p0, p1: O.Exponential(), "student_t": lambda p0, p1: O.StudentT(p0, p1), "gamma": lambda p0, p1: O.Gamma(p0),
          "beta": lambda p0, p1: O.Beta(p0)}


@pytest.mark.parametrize("kind", LR.KINDS)
def test_oracle_autograd_gradient_against_the_truth(kind):
    """the float64 oracle's variational_expectations and their torch-autograd gradient w.r.t. mean, variance and the likelihood's
    parameter, on the ordinary regime, within the bars the comparators set"""
    import torch
    case = element_case(f"{kind}-ordinary")
    T = LR.element_truth(case)
    n = case["mu"].size
    mu = torch.tensor(case["mu"].reshape(1, n, 1), requires_grad=True)
    v = torch.tensor(case["v"].reshape(1, n, 1), requires_grad=True)
    p0 = torch.tensor(case["p0"], dtype=torch.float64, requires_grad=True)
    ve = ORACLE[kind](p0, case["p1"]).variational_expectations(O.TH, mu, v, torch.tensor(case["y"].reshape(n, 1)))
    got = {"ve": ve.detach().numpy().ravel()}
    g = torch.autograd.grad(ve.sum(), [mu, v] + ([p0] if kind in LR.HAS_PARAM else []))
    got["dmu"], got["dv"] = g[0].numpy().ravel(), g[1].numpy().ravel()
    for q in ("ve", "dmu", "dv"):
        m = LR.measure(got[q], T["truth"][q])
        assert m <= T["bars"][q], (kind, q, m, T["bars"][q])
    if kind in LR.HAS_PARAM:      # autograd returns the SUM over the elements: its own n eps sum|terms| allowance
        val, sc = T["truth"]["dp0"]
        assert abs(float(g[2]) - float(val.sum())) <= (T["bars"]["dp0"] + n) * LR.EPS * float(sc.sum()), kind


def test_case_table_covers_the_listed_edges():
    by = {c["name"]: c for c in ELEMENT_CASES}
    for kind in LR.KINDS:
        assert set(SMALL_V) <= set(by[f"{kind}-small-v"]["v"]) and f"{kind}-ordinary" in by
    assert np.max(np.abs(by["bernoulli-large-mean-01"]["mu"])) == 12 and np.max(np.abs(by["beta-large-mean"]["mu"])) == 12
    assert set(by["bernoulli-large-mean-01"]["y"]) == {0.0, 1.0} and set(by["bernoulli-large-mean-pm1"]["y"]) == {-1.0, 1.0}
    for kind in ("exponential", "gamma"):
        c = by[f"{kind}-large-mean"]
        assert c["mu"].min() == -30 and c["mu"].max() == 30 and c["v"].max() == 20
    for b in (0.01, 1, 100):
        c = by[f"poisson-counts-binsize{b:g}"]
        assert set(POISSON_COUNTS) == set(c["y"]) and c["p1"] == b and c["mu"].max() == 30 and c["v"].max() == 20
    for sh in GAMMA_SHAPES:
        c = by[f"gamma-shape{sh:g}"]
        assert c["p0"] == sh and c["mu"][0] == 0.0 and c["y"][0] == 1.0
    for sc in BETA_SCALES:
        assert set(BETA_TARGETS) == set(by[f"beta-scale{sc:g}"]["y"])
    assert {c["p1"] for c in ELEMENT_CASES if c["kind"] == "student_t" and "nu" in c["name"]} == set(STUDENT_NU)
    assert {c["p0"] for c in ELEMENT_CASES if c["name"].startswith("gaussian-variance")} == {1e-6, 1.0, 1e6}
    Ks = {c["mean"].shape[2] for c in MULTICLASS_CASES}
    Rs = {c["mean"].shape[0] * c["mean"].shape[1] for c in MULTICLASS_CASES}
    assert {2, 3, 10, 31, 32} <= Ks and {1, 15, 16, 17, 33} <= Rs
    for c in MULTICLASS_CASES:
        K = c["mean"].shape[2]
        lab = c["labels"]
        assert lab.shape == (c["mean"].shape[1], 1) and np.all((lab >= 0) & (lab < K) & (lab == np.floor(lab))) and K - 1 in lab
    clips = next(c for c in MULTICLASS_CASES if c["name"] == "mc-clips-K3-R17")["var"]
    for x in (1e-10, np.nextafter(1e-10, 0), np.nextafter(1e-10, 1), 0.5e-10, np.nextafter(0.5e-10, 0), np.nextafter(0.5e-10, 1), 0.0):
        assert x in clips
    assert clips.min() < 0
    totals = {S * n * d for S, n, d in LAYOUT_SHAPES}
    assert {1, 255, 256, 257} <= totals and {d for _, _, d in LAYOUT_SHAPES} == {1, 2, 3, 20} and (1, 33, 20) in LAYOUT_SHAPES
    assert any((S * n) % 16 == 0 for S, n, _ in LAYOUT_SHAPES) and any((S * n) % 16 for S, n, _ in LAYOUT_SHAPES)
