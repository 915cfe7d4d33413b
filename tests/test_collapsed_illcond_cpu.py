"""-m "not gpu": the yardsticks of tests/test_gpu_collapsed_illcond.py on the three ill-conditioned cases of
tests/collapsed_reference.py (ILL_CASES), fed the float64 reference statistics in place of the device's.

Pinned here: the cases are as ill-conditioned as they are meant to be; the truth (collapsed_reference.truth: the chain with its
ill-conditioned part in double-longdouble) does not care about the order of the inducing inputs (1e-14 of each unit), so a
permutation is another float64 ORDER of the same problem; the family of six float64 orders
spreads over a factor that makes any single member useless as a yardstick; and the written-out float64 chain meets the stage bars the
device is held to (8 x the LAPACK chain's residual or the largest of the table).  Run with -s to read the figures."""
import numpy as np
import pytest

from tests import collapsed_reference as CR

_ST = {}


def _case(name):
    if name not in _ST:
        c = CR.ill_inputs(name)
        st = CR.float64_statistics(c)
        _ST[name] = (c, st, CR.truth(c, st))
    return _ST[name]


def _lapack_table():
    if "table" not in _ST:
        _ST["table"] = {n: CR.lapack_chain_residuals(*_case(n)[:2]) for n in CR.ILL_NAMES}
    return _ST["table"], np.max(np.stack(list(_ST["table"].values())), axis=0)


@pytest.mark.parametrize("name", CR.ILL_NAMES)
def test_cases_are_ill_conditioned(name):
    c, st, _ = _case(name)
    N, M, D, DY, noisy, ls, noise, seed = CR.ILL_CASES[name]
    assert c["mu"].shape == (N, D) and c["Z"].shape == (M, D) and c["Y"].shape == (N, DY) and (c["s"] is not None) == noisy
    cond = np.linalg.cond(st["Kuu"])
    Z = c["Z"]
    d = np.sqrt(np.sum((Z[:, None, :] - Z[None, :, :]) ** 2, axis=2)) + 1e9 * np.eye(M)
    print("%s: cond(Kuu + 1e-6 I) = %.3g, closest pair of inducing inputs %.3g lengthscales apart" % (name, cond, d.min() / ls))
    assert 1e6 <= cond <= 1e9
    assert d.min() < 0.5 * ls                      # what collapsed_reference.inputs keeps out
    if name == "pairs":
        assert np.max(np.abs(Z[M // 2:] - Z[:M // 2])) < 1e-3
    if name == "subset":
        assert np.array_equal(Z, c["mu"][:M]) and M > 128


def test_truth_is_permutation_invariant():
    """The truth on permuted inducing inputs against the one on the given order, every quantity in its unit: 1e-14.  The plain
    longdouble chain does not meet this at cond(Kuu) 2.5e7 .. 7e7 (cond x 2^-64 of rounding: it moves by up to 1.0e-12 on the mean,
    4.2e-14 on the variance, 2.7e-14 on the bound, and sits 3e-13 / 1.8e-14 / 2.7e-14 from the truth); with the ill-conditioned part
    of the chain in double-longdouble the permutations agree to the last longdouble bit (measured: 0 .. 3e-20)."""
    worst, plain = np.zeros(4), np.zeros(4)
    for name in CR.ILL_NAMES:
        c, st, truth = _case(name)
        M = st["Kuu"].shape[0]
        for k in (2, 3):
            perm = np.random.default_rng(1000 + k).permutation(M)
            e = np.array(CR.errors(CR.truth(c, st, perm=perm), truth, c))
            worst = np.maximum(worst, e)
            print("%s: truth under permutation %d moves by %s (bound, mean, var, cov)" % (name, k, " ".join("%.2g" % v for v in e)))
        e = np.array(CR.errors(CR.evaluate(c, st, CR.LD), truth, c))
        plain = np.maximum(plain, e)
        print("%s: the plain longdouble chain is %s from the truth" % (name, " ".join("%.2g" % v for v in e)))
    assert np.all(worst <= 1e-14), worst
    assert np.all(plain <= 1e-11)          # cond 1e8 x 2^-64 x the growth of a chain of six solves: the two chains are the same chain


@pytest.mark.parametrize("name", CR.ILL_NAMES)
def test_family_spreads(name):
    c, st, truth = _case(name)
    fam = CR.family_errors(c, st, truth)
    assert fam.shape == (CR.FAMILY, 4)
    lo, hi = fam.min(axis=0), fam.max(axis=0)
    for j, what in enumerate(("bound", "mean", "var", "cov")):
        print("%s %s: family of %d float64 orders %.3g .. %.3g (spread %.1f x)" % (name, what, CR.FAMILY, lo[j], hi[j], hi[j] / lo[j]))
    assert np.all(hi < 1e-6) and np.all(lo > 0)
    assert hi[0] / lo[0] >= 3.0                     # no single order is the rounding level of the bound


@pytest.mark.parametrize("name", CR.ILL_NAMES)
def test_written_out_chain_meets_the_stage_bars(name):
    c, st, _ = _case(name)
    table, worst = _lapack_table()
    print("LAPACK chain, largest over the cases: " + "  ".join("%s %.3g" % (s, w) for s, w in zip(CR.STAGES + CR.PREDICT_STAGES, worst)))
    lo = CR.evaluate(c, st, np.float64)["state"]
    tmp1 = CR.solve_lower(lo["L"], st["Kus"])
    tmp2 = CR.solve_lower(lo["LB"], tmp1)
    got = np.concatenate([CR.stage_residuals(st, c["Y"], c["noise"], lo["L"], lo["G"], lo["LB"], lo["c"]),
                          CR.predict_residuals(st["Kus"], lo["L"], lo["LB"], tmp1, tmp2)])
    for j, what in enumerate(CR.STAGES + CR.PREDICT_STAGES):
        bar = 8.0 * max(table[name][j], worst[j])
        print("%s  %s: written-out %.3g, LAPACK %.3g, bar %.3g (units of 2^-53)" % (name, what, got[j], table[name][j], bar))
        assert got[j] <= bar
        assert table[name][j] <= 64.0              # the LAPACK chain itself is backward stable, stage by stage


def test_assembly_terms_are_the_terms():
    c, st, _ = _case("pairs")
    truth = CR.evaluate(c, st, CR.LD)
    s = truth["state"]
    t = CR.assembly_terms(s["LB"], s["G"], s["c"], c["Y"], st["psi0"], c["noise"])
    assert float(np.max(np.abs(t - truth["terms"]))) <= 2.0 ** -60 * float(np.sum(np.abs(truth["terms"])))


def test_collapsed_is_collapsed_from():
    """collapsed() is collapsed_from() on its own statistics: the well-conditioned yardstick keeps its bits"""
    c = CR.inputs("n40")
    lo = CR.state("n40", np.float64)
    st = CR.float64_statistics(c)
    again = CR.collapsed_from(st["Kuu"], st["psi0"], st["psi1"], st["psi2"], c["Y"], c["noise"], np.float64)
    assert again["bound"] == lo["bound"] and np.array_equal(again["LB"], lo["LB"]) and np.array_equal(again["c"], lo["c"])
