"""CPU-side checks of the greedy inducing-point yardstick (tests/greedy_reference.py on the cases of tests/greedy_cases.py) and of
everything layer_initializations.greedy_inducing / DGP(..., inducing=...) refuse before a device is looked for.

Bounds.  L L^T = k(Z, Z) (+ White): column b of row a is (k - sum_{t<b} ...) / sqrt(res_b) times sqrt(res_b), and the diagonal is d
lowered one c^2 at a time, so the product misses k by roundings only, never by an amplified error: (m + 4) 2^-52 (v + white) per entry.
trace_j against tr(K - K_.S K_SS^-1 K_S.) by a float64 solve: the solve's own error is about cond(K_SS) 2^-53 of the n v it is
subtracted from; 64 cond(K_SS) 2^-53 n v is allowed."""
import numpy as np
import pytest

from tests import greedy_cases as GC
from tests import greedy_reference as R


@pytest.mark.parametrize("name", GC.NAMES)
def test_reference_pins_the_rows_and_factorises_kzz(name):
    c = GC.inputs(name)
    ref, f64 = GC.reference(name), GC.float64(name)
    print("%s: m = %d, margin %.3g" % (name, ref["m"], ref["margin"]))
    assert ref["margin"] >= GC.MARGIN, "the case does not pin its rows: another seed"
    assert ref["m"] == f64["m"] and np.array_equal(ref["indices"], f64["indices"])
    assert len(set(ref["indices"].tolist())) == ref["m"]
    if c["first"] is not None:
        assert ref["indices"][0] == c["first"] != 0
    m = ref["m"]
    bound = (m + 4) * 2.0 ** -52 * (c["v"] + c["white"])
    for run, dtype in ((ref, R.LD), (f64, np.float64)):
        Z = c["X"][run["indices"]].astype(dtype)
        K = R.kernel_matrix(Z, c["kind"], c["v"], c["ls"].astype(dtype), c["white"])
        Lw = run["L"].astype(R.LD)
        err = float(np.abs(Lw @ Lw.T - K.astype(R.LD)).max())
        print("  %s: |L L^T - k(Z, Z)| %.3g (bound %.3g)" % (np.dtype(dtype).name, err, bound))
        assert np.all(np.triu(run["L"], 1) == 0) and err <= bound
    assert np.all(np.diff(ref["trace"].astype(np.float64)) <= 0) and np.all(ref["residual"] > c["threshold"])


@pytest.mark.parametrize("name", ["a", "tiny", "dup"])
def test_trace_is_the_trace_of_kff_minus_qff(name):
    c = GC.inputs(name)
    ref = GC.reference(name)
    X, n = c["X"], c["X"].shape[0]
    K = R.kernel_matrix(X, c["kind"], c["v"], c["ls"], c["white"])
    for j in (0, ref["m"] // 2, ref["m"] - 1):
        S = ref["indices"][:j + 1]
        Kss, Ksx = K[np.ix_(S, S)], K[S]
        direct = np.trace(K) - np.sum(Ksx * np.linalg.solve(Kss, Ksx))
        bound = 64 * np.linalg.cond(Kss) * 2.0 ** -53 * n * c["v"]
        print("%s, %d points: trace %.6g, direct %.6g, bound %.3g" % (name, j + 1, float(ref["trace"][j]), direct, bound))
        assert abs(float(ref["trace"][j]) - direct) <= bound


def test_duplicated_rows_stop_at_the_distinct_ones():
    c = GC.inputs("dup")
    ref = GC.reference("dup")
    assert ref["m"] == 20 < c["M"]
    assert len({c["X"][i].tobytes() for i in ref["indices"]}) == 20 == len({r.tobytes() for r in c["X"]})
    assert float(ref["residual"][-1]) > 1e-3 and len(ref["margins"]) == 21      # the 21st step met the threshold


def test_bad_arguments_raise_before_a_device_is_looked_for():
    from doubly_stochastic_dgp.gpflow_compat import RBF, Matern52, White, Kernel
    from doubly_stochastic_dgp.layer_initializations import greedy_inducing
    X = np.array(GC.inputs("a")["X"])
    k = RBF(3)
    bad = X.copy()
    bad[5, 1] = np.nan

    class Periodic(Kernel):
        input_dim = 3

    for args, kw in (((X[:, 0], 10, RBF(1)), {}), ((X, 1, k), {}), ((X, 2049, k), {}), ((X, 601, k), {}), ((X, 10.0, k), {}),
                     ((X, True, k), {}), ((np.zeros((40, 1025)), 10, RBF(1025)), {}), ((np.zeros((40, 0)), 10, k), {}),
                     ((X, 10, k), dict(first=-1)), ((X, 10, k), dict(first=600)), ((X, 10, k), dict(first=1.5)),
                     ((X, 10, k), dict(threshold=-1e-9)), ((X, 10, k), dict(threshold=float("nan"))), ((bad, 10, k), {}),
                     ((X, 10, RBF(4)), {}), ((X, 10, Periodic()), {}), ((X, 10, White(3)), {}), ((X, 10, RBF(3) + Matern52(3)), {})):
        with pytest.raises(ValueError):
            greedy_inducing(*args, **kw)


def test_dgp_refuses_an_unknown_inducing_rule():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    X = np.array(GC.inputs("a")["X"])
    Y = np.zeros((X.shape[0], 1))
    with pytest.raises(ValueError, match="nonsense"):
        DGP(X, Y, 10, [RBF(3), RBF(3)], Gaussian(), inducing="nonsense")
